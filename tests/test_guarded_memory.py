"""Every operator in guarded memory (tests/guarded.py): stray stores, stray loads, unwritten output, dependence on what the output held.

A case builds its inputs from seeded host tensors with Guard.tensor, calls the public Python wrapper and returns the tensors the caller
gets back (outputs, gradients, records), with a mask where the header leaves a region unspecified.  The test runs it plain, guarded
with nan / 0x5A and guarded with -12345.678 / 0xA5, and asserts
  (a) no guard byte changed in either guarded run;
  (b) the two guarded runs agree bit for bit inside the specified regions;
  (c) they agree bit for bit with the plain run (the library's sums have a fixed order) -- which ties them to the float64 comparisons
      the plain calls pass in the operators' own tests;
  (d) every device pointer the library was given lay in guarded memory, but for the arguments the case declares with a reason.
Shapes: the smallest at which the access pattern changes, taken from the border tables of the operators' own tests.  The last test
asserts from the call log that every entry point that takes a caller's tensor was reached.  No tolerance anywhere.
"""
import copy
import ctypes as ct
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))

import guarded                                    # noqa: E402
from fastdiff_amd import _capi                    # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = {}          # id -> (function, {(entry point, argument index): reason})
REPORTS = {}        # id -> guarded.Report of the cases that have run in this process

HOST_BANK = "a host array (numpy) into which the wrapper itself reads the handle's filter bank; the library uses it on the host"
HOST_PINV ="a host array (numpy) the wrapper computes itself from the handle's filter bank; the library reads it on the host"


def case(name, declared=None):
    def put(fn):
        assert name not in CASES
        CASES[name] = (fn, declared or {})
        return fn
    return put


def rnd(seed, *shape, scale=1.0):
    return scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def leaf(g, t):
    return g.tensor(t).requires_grad_(True)


def grads(outs, inputs, gouts):
    return torch.autograd.grad(outs, inputs, gouts)


def as_tensors(record, prefix=""):
    return {prefix + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in record.items()}


_model = None


def model():
    """The inference module of the parity tests, made (and its weights uploaded) outside every guarded context: a case's plain run
    comes first."""
    global _model
    if _model is None:
        import gpu_common
        _model = gpu_common.make_model()
    return _model


_rows = None


def rows2():
    """A two-step schedule (the last two betas of the reference's N = 4 list)."""
    global _rows
    if _rows is None:
        from fastdiff_amd import sampler, schedules
        _rows = sampler.InferenceSchedule(schedules.training_hyperparams(), torch.FloatTensor([2.5376e-02, 7.0414e-01]), verbose=False).rows()
    return _rows


# =====================================================================================================================================
# Training operators (fastdiff_amd.lvc_op): forward and every gradient
# =====================================================================================================================================
def _lvc(name, B, T, hop, Cin=32, Cout=64, ks=3):
    @case(name)
    def fn(g):
        import fastdiff_amd
        x, K = leaf(g, rnd(1, B, Cin, T * hop)), leaf(g, rnd(2, B, Cin, Cout, ks, T, scale=0.2))
        b, d = leaf(g, rnd(3, B, Cout, T)), g.tensor(rnd(4, B, Cout, T * hop))
        y = fastdiff_amd.location_variable_convolution(x, K, b, 1, hop)
        dx, dK, db = grads(y, (x, K, b), d)
        return {"out": y, "dx": dx, "dK": dK, "db": db}


for _hop in (8, 64, 256):
    _lvc(f"lvc-hop{_hop}-1x1", 1, 1, _hop)
    _lvc(f"lvc-hop{_hop}-3x65", 3, 65, _hop)
_lvc("lvc-generic-2x7", 2, 7, 12, Cin=6, Cout=10, ks=5)          # test_other_shapes_take_the_generic_kernels


def _lvc_slices(name, B, T, layers, hop):
    @case(name)
    def fn(g):
        import fastdiff_amd
        from fastdiff_amd import lvc_op
        k6 = leaf(g, rnd(5, B, layers, 32, 64, 3, T, scale=0.1))
        slices, slots = lvc_op.split_layers(k6)
        xs = [leaf(g, rnd(10 + i, B, 32, T * hop)) for i in range(layers)]
        bs = [leaf(g, rnd(20 + i, B, 64, T)) for i in range(layers)]
        ds = [g.tensor(rnd(30 + i, B, 64, T * hop)) for i in range(layers)]
        ys = [fastdiff_amd.location_variable_convolution(xs[i], slices[i], bs[i], 1, hop, grad_slot=slots[i]) for i in range(layers)]
        got = grads(ys, [k6] + xs + bs, ds)
        out = {"dK6": got[0]}
        for i in range(layers):
            out.update({f"out{i}": ys[i], f"dx{i}": got[1 + i], f"db{i}": got[1 + layers + i]})
        return out


_lvc_slices("lvc-slices-2x1x2", 2, 1, 2, 256)
_lvc_slices("lvc-slices-2x37x4", 2, 37, 4, 8)


def _lvc_frames(name, B, T, layers, hop, dx_mode):
    @case(name)
    def fn(g):
        from fastdiff_amd import lvc_op
        lib, h = lvc_op._handle(torch.device(DEV, torch.cuda.current_device()))
        assert lib.fd_set_option(h, b"lvc_dx", dx_mode.encode()) == 0
        try:
            fr = leaf(g, lvc_op.reference_to_frames(rnd(5, B, layers, 32, 64, 3, T, scale=0.1), "forward"))
            bias = leaf(g, rnd(6, B, layers, 64, T))
            slices, slots = lvc_op.split_layers(fr)
            bslices, bslots = lvc_op.split_layers(bias)
            xs = [leaf(g, rnd(10 + i, B, 32, T * hop)) for i in range(layers)]
            ds = [g.tensor(rnd(30 + i, B, 64, T * hop)) for i in range(layers)]
            ys = [lvc_op.location_variable_convolution_frames(xs[i], slices[i], bslices[i], hop, grad_slot=slots[i], bias_slot=bslots[i])
                  for i in range(layers)]
            got = grads(ys, [fr, bias] + xs, ds)
        finally:
            assert lib.fd_set_option(h, b"lvc_dx", b"gather") == 0
        out = {"dframes": got[0], "dbias": got[1]}
        for i in range(layers):
            out.update({f"out{i}": ys[i], f"dx{i}": got[2 + i]})
        return out


for _mode in ("gather", "copy"):
    _lvc_frames(f"lvc-frames-2x1x2-{_mode}", 2, 1, 2, 256, _mode)
    _lvc_frames(f"lvc-frames-2x37x4-{_mode}", 2, 37, 4, 8, _mode)


def _gate(name, B, C, L):
    @case(name)
    def fn(g):
        import fastdiff_amd
        x, y, d = leaf(g, rnd(1, B, C, L)), leaf(g, rnd(2, B, 2 * C, L, scale=4.0)), g.tensor(rnd(3, B, C, L))
        out = fastdiff_amd.gated_residual(x, y)
        (dy,) = grads(out, (y,), d)
        return {"out": out, "dy": dy}


_gate("gate-3x5x37", 3, 5, 37)
_gate("gate-1x32x56", 1, 32, 56)


def _kconv(name, M, B, T, slope):
    @case(name)
    def fn(g):
        import fastdiff_amd
        x, w, b = leaf(g, rnd(1, B, 64, T)), leaf(g, rnd(2, M, 64, 3, scale=1 / 14)), leaf(g, rnd(3, M))
        d = g.tensor(rnd(4, B, M, T))
        y = fastdiff_amd.kernel_conv1d(x, w, b, slope)
        dx, dw, db = grads(y, (x, w, b), d)
        return {"out": y, "dx": dx, "dw": dw, "db": db}


_kconv("kconv-M32-T1-act", 32, 2, 1, 0.1)
_kconv("kconv-M32-T37", 32, 2, 37, 1.0)
_kconv("kconv-M96-T37-act", 96, 2, 37, 0.1)
_kconv("kconv-M96-T128", 96, 1, 128, 1.0)
_kconv("kconv-M384-T1", 384, 3, 1, 1.0)
_kconv("kconv-M384-T128-act", 384, 2, 128, 0.1)
_kconv("kconv-large-640x1x1", 640, 1, 1, 1.0)          # two rows of KCONV_CASES (M, B, T): one frame; T % 4 = 2 next to a boundary
_kconv("kconv-large-544x2x2", 544, 2, 2, 1.0)


def _kconv_frames(name, B, T, layers):
    @case(name)
    def fn(g):
        from fastdiff_amd import lvc_op
        M = layers * lvc_op.FRAME
        x, w, b = leaf(g, rnd(1, B, 64, T)), leaf(g, rnd(2, M, 64, 3, scale=1 / 14)), leaf(g, rnd(3, M))
        d = g.tensor(rnd(4, B, layers, T, lvc_op.FRAME))
        y = lvc_op.kernel_conv1d_frames(x, w, b)
        dx, dw, db = grads(y, (x, w, b), d)
        return {"out": y, "dx": dx, "dw": dw, "db": db}


_kconv_frames("kconv-frames-1x1x1", 1, 1, 1)
_kconv_frames("kconv-frames-3x33x4", 3, 33, 4)


def _stack(name, B, T, n):
    @case(name)
    def fn(g):
        from fastdiff_amd import lvc_op
        x = leaf(g, rnd(1, B, 64, T))
        ws = [leaf(g, rnd(10 + j, 64, 64, 3, scale=1 / 14)) for j in range(n)]
        bs = [leaf(g, rnd(20 + j, 64)) for j in range(n)]
        y = lvc_op.kernel_conv_stack(x, ws, bs, 0.1)
        got = grads(y, [x] + ws + bs, g.tensor(rnd(2, B, 64, T)))
        out = {"out": y, "dx": got[0]}
        for j in range(n):
            out.update({f"dw{j}": got[1 + j], f"db{j}": got[1 + n + j]})
        return out


_stack("stack-2x1x3", 2, 1, 3)
_stack("stack-2x37x2", 2, 37, 2)


@case("fronts-8x3x2x5")
def _fronts(g, P=8, n=3, B=2, T=5):
    from fastdiff_amd import lvc_op
    xs = [leaf(g, rnd(100 + p, B, 80, T)) for p in range(P)]
    ics = [(leaf(g, rnd(200 + p, 64, 80, 5, scale=1 / 20)), leaf(g, rnd(300 + p, 64))) for p in range(P)]
    sts = [[(leaf(g, rnd(400 + 10 * p + j, 64, 64, 3, scale=1 / 14)), leaf(g, rnd(500 + 10 * p + j, 64))) for j in range(n)] for p in range(P)]
    ys = lvc_op.predictor_fronts(xs, ics, sts, 0.1)
    params = [t for p in range(P) for t in (*ics[p], *[t for pair in sts[p] for t in pair])]
    got = grads(ys, xs + params, [g.tensor(rnd(600 + p, B, 64, T)) for p in range(P)])
    out = {f"out{p}": ys[p] for p in range(P)}
    out.update({f"grad{i}": t for i, t in enumerate(got)})
    return out


@case("side-by-side-8x96x1x5")
def _side(g, P=8, M=96, B=1, T=5):
    from fastdiff_amd import lvc_op
    xs = [leaf(g, rnd(100 + p, B, 64, T)) for p in range(P)]
    ws = [leaf(g, rnd(200 + p, M, 64, 3, scale=1 / 14)) for p in range(P)]
    bs = [leaf(g, rnd(300 + p, M)) for p in range(P)]
    ys = lvc_op.kernel_conv1d_side_by_side(xs, ws, bs)
    got = grads(ys, xs + ws + bs, [g.tensor(rnd(600 + p, B, M, T)) for p in range(P)])
    out = {f"out{p}": ys[p] for p in range(P)}
    out.update({f"grad{i}": t for i, t in enumerate(got)})
    return out


def _fan(name, B, L, f):
    @case(name)
    def fn(g):
        from fastdiff_amd import lvc_op
        x = leaf(g, rnd(1, B, 32, L))
        outs = lvc_op.skip_fan(x, f)
        gouts = [g.tensor(rnd(2, B, 32, L // f))] + [g.tensor(rnd(3 + i, B, 32, L)) for i in range(4)]
        (dx,) = grads(outs, (x,), gouts)
        return {"picked": outs[0], "dx": dx}


_fan("fan-1x8x8", 1, 8, 8)
_fan("fan-2x30x3", 2, 30, 3)


def _input_conv(name, B, T):
    @case(name)
    def fn(g):
        from fastdiff_amd import lvc_op
        x, w, b = leaf(g, rnd(1, B, 80, T)), leaf(g, rnd(2, 64, 80, 5, scale=1 / 20)), leaf(g, rnd(3, 64))
        y = lvc_op.input_conv(x, w, b, 0.1)
        dx, dw, db = grads(y, (x, w, b), g.tensor(rnd(4, B, 64, T)))
        return {"out": y, "dx": dx, "dw": dw, "db": db}


_input_conv("input-conv-T1", 2, 1)
_input_conv("input-conv-T9", 3, 9)
_input_conv("input-conv-T37", 3, 37)


def _two_smallest(table, size):
    return sorted(table, key=size)[:2]


import test_training_convs_f64 as _convs          # noqa: E402  (the border tables of the three small convolutions)


def _conv32(name, B, L, dil, skip, post):
    @case("conv32-" + name)
    def fn(g):
        from fastdiff_amd import lvc_op
        x, w, b = leaf(g, rnd(1, B, 32, L)), leaf(g, rnd(2, 32, 32, 3, scale=0.1)), leaf(g, rnd(3, 32))
        s = leaf(g, rnd(4, B, 32, L)) if skip else None
        res = lvc_op.conv32(x, w, b, dil, skip=s, post_slope=post)
        outs = list(res) if skip else [res]
        ins = [x, w, b] + ([s] if skip else [])
        got = grads(outs, ins, [g.tensor(rnd(5 + i, B, 32, L)) for i in range(len(outs))])
        out = {f"out{i}": t for i, t in enumerate(outs)}
        out.update({f"grad{i}": t for i, t in enumerate(got)})
        return out


for _c in _two_smallest(_convs.CONV32_CASES, lambda c: c[1] * c[2]):
    _conv32(*_c)
_conv32("wave-L28-noskip", 2, 28, 1, False, 1.0)          # (the table's first row without its skip: the other forward signature)


def _conv7(name, which, B, L):
    @case("conv7-" + name)
    def fn(g):
        from fastdiff_amd import lvc_op
        cin, cout = (1, 32) if which == 0 else (32, 1)
        x, w, b = leaf(g, rnd(1, B, cin, L)), leaf(g, rnd(2, cout, cin, 7, scale=0.2)), leaf(g, rnd(3, cout))
        y = lvc_op.conv7(x, w, b)
        dx, dw, db = grads(y, (x, w, b), g.tensor(rnd(4, B, cout, L)))
        return {"out": y, "dx": dx, "dw": dw, "db": db}


for _which in (0, 1):
    for _c in _two_smallest([c for c in _convs.CONV7_CASES if c[1] == _which], lambda c: c[2] * c[3]):
        _conv7(*_c)


def _upsample(name, B, Lin, r):
    @case("upsample-" + name)
    def fn(g):
        from fastdiff_amd import lvc_op
        x, w, b = leaf(g, rnd(1, B, 32, Lin)), leaf(g, rnd(2, 32, 32, 2 * r, scale=1 / 8)), leaf(g, rnd(3, 32))
        y = lvc_op.upsample(x, w, b, r)
        dx, dw, db = grads(y, (x, w, b), g.tensor(rnd(4, B, 32, Lin * r)))
        return {"out": y, "dx": dx, "dw": dw, "db": db}


for _r in (8, 4):
    for _c in _two_smallest([c for c in _convs.UPSAMPLE_CASES if c[3] == _r], lambda c: c[1] * c[2]):
        _upsample(*_c)


def _weight_norm(name, shape):
    @case(name)
    def fn(g):
        from fastdiff_amd import lvc_op
        v, gg = leaf(g, rnd(1, *shape)), leaf(g, torch.rand(shape[0], 1, 1, generator=torch.Generator().manual_seed(2)) + 0.5)
        w = lvc_op.weight_norm(v, gg)
        dv, dg = grads(w, (v, gg), g.tensor(rnd(3, *shape)))
        return {"w": w, "dv": dv, "dg": dg}


_weight_norm("weight-norm-32x1x7", (32, 1, 7))
_weight_norm("weight-norm-1x32x7", (1, 32, 7))
_weight_norm("weight-norm-64x80x5", (64, 80, 5))


@case("weight-norm-all")
def _weight_norm_all(g):
    """30 tensors of the model's shapes: more than the 28 records of one launch."""
    from fastdiff_amd import lvc_op
    shapes = [(256, 64, 3), (64, 80, 5), (32, 1, 7), (1, 32, 7), (32, 32, 1)] + [(64, 64, 3)] * 10 + [(32, 32, 3)] * 15
    gen = torch.Generator().manual_seed(4)
    vs = [leaf(g, torch.randn(*sh, generator=gen)) for sh in shapes]
    gs = [leaf(g, torch.rand(sh[0], 1, 1, generator=gen) + 0.5) for sh in shapes]
    ws = lvc_op.weight_norm_all(list(zip(vs, gs)))
    got = grads(ws, vs + gs, [g.tensor(torch.randn(*sh, generator=gen)) for sh in shapes])
    out = {f"w{i}": w for i, w in enumerate(ws)}
    out.update({f"grad{i}": t for i, t in enumerate(got)})
    return out


@case("raw-lvc-and-kconv")
def _raw(g, B=2, T=5, hop=8, M=64):
    """The entry points without a batch stride or an activation, which the wrappers reach only through their wider twins
    (fd_lvc_forward / _backward, fd_kconv_forward / _backward), called as the header declares them."""
    from fastdiff_amd import lvc_op
    dev = torch.device(DEV, torch.cuda.current_device())
    x, K, b, d = (g.tensor(t) for t in (rnd(1, B, 32, T * hop), rnd(2, B, 32, 64, 3, T, scale=0.2), rnd(3, B, 64, T), rnd(4, B, 64, T * hop)))
    out, dx, dK, db = (torch.empty_like(t) for t in (d, x, K, b))
    lvc_op._call(dev, "fd_lvc_forward", "fd_lvc_forward", x, K, b, B, 32, 64, 3, T, hop, out)
    lvc_op._call(dev, "fd_lvc_backward", "fd_lvc_backward", x, K, d, B, 32, 64, 3, T, hop, dx, dK, db)
    cx, w, cb, cd = (g.tensor(t) for t in (rnd(5, B, 64, T), rnd(6, M, 64, 3, scale=1 / 14), rnd(7, M), rnd(8, B, M, T)))
    cout, cdx, cdw, cdb = (torch.empty_like(t) for t in (cd, cx, w, cb))
    lvc_op._call(dev, "fd_kconv_forward", "fd_kconv_forward", cx, w, cb, B, M, T, cout)
    lvc_op._call(dev, "fd_kconv_backward", "fd_kconv_backward", cx, w, cd, B, M, T, cdx, cdw, cdb)
    return {"out": out, "dx": dx, "dK": dK, "db": db, "cout": cout, "cdx": cdx, "cdw": cdw, "cdb": cdb}


# =====================================================================================================================================
# The step: draws, loss, distances, optimizer, collaters, the evaluation's sums
# =====================================================================================================================================
def _alpha():
    from fastdiff_amd import schedules
    return schedules.training_hyperparams()["alpha"].detach().float().cpu()


def _draws(name, B, L=256):
    @case("train-draw-" + name)
    def fn(g):
        from fastdiff_amd import lvc_op
        x0, alpha = g.tensor(rnd(1, B, 1, L, scale=0.3)), g.tensor(_alpha())
        x_t, z, steps = lvc_op.train_draw(x0, alpha, 1000, seed=1234, iteration=3)
        state = lvc_op.new_train_state(x0.device)
        by_state = lvc_op.train_draw(x0, alpha, 1000, seed=1234, iteration=0, state=state)
        return {"x_t": x_t, "z": z, "steps": steps, "x_t state": by_state[0], "z state": by_state[1], "steps state": by_state[2]}

    @case("phi-draw-" + name)
    def fn2(g):
        from fastdiff_amd import lvc_op
        x0, alpha = g.tensor(rnd(1, B, 1, L, scale=0.3)), g.tensor(_alpha())
        names = ("x_t", "z", "steps", "beta_nxt", "delta", "delta2")
        return dict(zip(names, lvc_op.phi_draw(x0, alpha, 1000, 200, seed=1234, iteration=3)))


_draws("B1", 1)
_draws("B5", 5)


def _mse(n):
    @case(f"mse-n{n}")
    def fn(g):
        from fastdiff_amd import lvc_op
        eps, z = leaf(g, rnd(1, 1, 1, n)), g.tensor(rnd(2, 1, 1, n))
        state = lvc_op.new_train_state(eps.device)
        loss = lvc_op.mse_loss(eps, z, state)
        (deps,) = grads(loss, (eps,), g.tensor(torch.tensor(1.5)))
        return {"loss": loss, "deps": deps, "state": state}


for _n in (4095, 4096, 4097):          # around FD_STEP_RUN * 256
    _mse(_n)


def _distance(n):
    @case(f"item-distance-n{n}")
    def fn(g):
        from fastdiff_amd import lvc_op
        a, b = g.tensor(rnd(1, 3, n)), g.tensor(rnd(2, 3, n))
        return {"l2": lvc_op.item_distance(a, b, 0), "l1": lvc_op.item_distance(a, b, 1)}


_distance(3)
_distance(4097)


def _adamw(name):
    @case("adamw-" + name)
    def fn(g):
        """The model's 175 parameter shapes as tests/test_train_step.py steps them; one item without a gradient."""
        import test_train_step as tts
        from fastdiff_amd import lvc_op
        gscale, max_norm = {c[0]: c[1:] for c in tts.CASES}[name]
        shapes = tts._shapes()
        P = [g.tensor(t) for t in tts._hash_tensors(77, 1, shapes, 0.1, DEV)]
        G = [g.tensor(t) for t in tts._hash_tensors(77, 10, shapes, gscale, DEV)]
        M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
        hyper = g.tensor(torch.tensor([2e-4, 0.9, 0.98, 1e-8, 0.01, max_norm], dtype=torch.float64))
        st = lvc_op.new_train_state(DEV)
        lvc_op.adamw_multi([(p, None if i == tts.FROZEN else gi, m, v) for i, (p, gi, m, v) in enumerate(zip(P, G, M, V))], hyper, st)
        out = {"state": st}
        for i in range(len(P)):
            out.update({f"p{i}": P[i], f"m{i}": M[i], f"v{i}": V[i]})
        return out


_adamw("above")
_adamw("below")


def _collaters(F):
    def corpus(g, kind):
        import test_train_corpus as ttc
        from fastdiff_amd.corpus import TrainCorpus
        cpu = TrainCorpus(ttc.make_items(ttc._lengths(kind, F), 256, seed=F), hop_size=256, max_samples=F * 256, device="cpu")
        c = copy.copy(cpu)
        c.mel, c.wav, c.frame_off = g.tensor(cpu.mel), g.tensor(cpu.wav), g.tensor(cpu.frame_off)
        c.device = c.wav.device
        return c

    @case(f"train-collate-F{F}")
    def fn(g):
        from fastdiff_amd import lvc_op
        mels, wavs, picked = lvc_op.train_collate(corpus(g, "three"), 5, seed=1234, iteration=1)
        return {"mels": mels, "wavs": wavs, "picked": picked}

    @case(f"eval-collate-F{F}")
    def fn2(g):
        from fastdiff_amd import lvc_op
        mels, wavs, picked = lvc_op.eval_collate(corpus(g, "three"), 5, seed=1234, iteration=0)          # (3 items in 5 slots: two fillers)
        return {"mels": mels, "wavs": wavs, "picked": picked}


_collaters(7)
_collaters(33)


@case("eval-accumulate-7x1")
def _eval_accumulate(g, B=5):
    from fastdiff_amd import lvc_op
    values = g.tensor(rnd(1, B).abs())
    picked = g.tensor(torch.tensor([[0, 0], [1, 0], [2, 0], [-1, -1], [4, 0]], dtype=torch.int64))
    steps = g.tensor(torch.tensor([0.0, 3.0, 6.0, 1.0, 2.0]))
    acc, item_out, state = lvc_op.new_eval_state(DEV), torch.zeros(B, device=DEV), lvc_op.new_train_state(DEV)
    lvc_op.eval_accumulate(values, picked, acc, steps=steps, T_train=7, bins=1, item_out=item_out, advance=state)
    return {"acc": acc, "item_out": item_out, "state": state}


# =====================================================================================================================================
# The scheduling network
# =====================================================================================================================================
def _band_pool(L):
    @case(f"band-pool-L{L}")
    def fn(g):
        from fastdiff_amd import lvc_op
        x, w, b = g.tensor(rnd(1, 2, L)), leaf(g, rnd(2, 32, 64, scale=0.1)), leaf(g, rnd(3, 32, scale=0.1))
        feat = lvc_op.band_pool(x, w, b)
        dW, db = grads(feat, (w, b), g.tensor(rnd(4, 2, 32)))
        return {"feat": feat, "dW": dW, "db": db}


for _L in (64, 96, 32 * 128, 32 * 130):
    _band_pool(_L)


def _head(name, B, R):
    @case("npred-head-" + name)
    def fn(g):
        from fastdiff_amd import lvc_op
        feat = leaf(g, rnd(1, B, 32))
        beta_next, delta2 = g.tensor(torch.rand(R, generator=torch.Generator().manual_seed(2)) * 0.1 + 0.01), g.tensor(torch.full((R,), 0.3))
        w1, b1, w2, b2 = leaf(g, rnd(3, 64, 34, scale=0.2)), leaf(g, rnd(4, 64, scale=0.2)), leaf(g, rnd(5, 1, 64, scale=0.2)), leaf(g, rnd(6, 1))
        out = {}
        if R == B:
            beta_hat, ratio = lvc_op.npred_head(feat, beta_next, delta2, w1, b1, w2, b2)
            got = grads(beta_hat, (feat, w1, b1, w2, b2), g.tensor(rnd(7, R)))
            out.update({f"grad{i}": t for i, t in enumerate(got)})
        else:
            with torch.no_grad():
                beta_hat, ratio = lvc_op.npred_head(feat, beta_next, delta2, w1, b1, w2, b2)
        out.update({"beta_hat": beta_hat, "ratio": ratio})
        return out


_head("B1", 1, 1)
_head("B3", 3, 3)
_head("B3-R1", 3, 1)


def _phi_residual(L):
    @case(f"phi-residual-L{L}")
    def fn(g):
        from fastdiff_amd import lvc_op
        eps, z = g.tensor(rnd(1, 3, 1, L)), g.tensor(rnd(2, 3, 1, L))
        delta, beta_hat = g.tensor(torch.tensor([0.2, 0.5, 0.9])), leaf(g, torch.tensor([0.01, 0.1, 0.3]))
        m = lvc_op.phi_residual(eps, z, delta, beta_hat)
        (dbeta,) = grads(m, (beta_hat,), g.tensor(rnd(3, 3)))
        return {"m": m, "dbeta": dbeta}


_phi_residual(256)
_phi_residual(4100)


@case("sched-update-n1025-refused-n4100")
def _sched(g):
    """n = 1025 is not a multiple of 4: fd_sched_update refuses it (fd_api_train.cpp) and must then touch nothing; n = 4100 is 1025
    16-byte vectors, phi_residual's border."""
    from fastdiff_amd import lvc_op
    alpha = g.tensor(_alpha())
    state = lvc_op.new_sched_state(torch.device(DEV, torch.cuda.current_device()), 0.5, 0.7)
    steps, cond = torch.zeros((1, 1), device=DEV, dtype=torch.float32), g.tensor(torch.tensor([0.5, 1.0]))
    lvc_op.sched_begin(state, None, 0.5, alpha, False, steps)
    odd_x, odd_eps = g.tensor(rnd(1, 1, 1, 1025)), g.tensor(rnd(2, 1, 1, 1025))
    with pytest.raises(AssertionError, match="multiple of 4"):
        lvc_op.sched_update(state, odd_x, odd_eps, cond)
    out = {"state refused": state.clone(), "cond refused": cond.clone(), "x refused": odd_x}
    x, eps = g.tensor(rnd(1, 1, 1, 4100)), g.tensor(rnd(2, 1, 1, 4100))
    lvc_op.sched_update(state, x, eps, cond)
    lvc_op.sched_begin(state, g.tensor(torch.tensor([0.2])), 0.5, alpha, False, steps)
    out.update({"state": state, "steps": steps, "cond": cond, "x": x})
    return out


# =====================================================================================================================================
# Waveform tools: batches of 3 with `valid`, the shortest item first and last
# =====================================================================================================================================
def _wave(seed, B, n, scale=0.3):
    return rnd(seed, B, n, scale=scale).clamp_(-1, 1)


def _ragged(name, lengths):
    """(suffix, valid) for the shortest item first and for it last; `lengths` ascending."""
    return ((name + "-short-first", list(lengths)), (name + "-short-last", list(lengths[::-1])))


def _padded(t, valid, per=1):
    """The zero-padded batch the `valid` contract speaks of."""
    for b, v in enumerate(valid):
        t[b, v * per:] = 0
    return t


def _mel(variant):
    @case(f"mel-spectrogram-{variant}")
    def fn(g):
        m = model()
        out = {}
        for n in (513, 700, 1024):
            out[f"mel{n}"] = m.mel_spectrogram(g.tensor(_wave(n, 3, n)), variant=variant)
        out["mel1024-3frames"] = m.mel_spectrogram(g.tensor(_wave(5, 3, 1024)), n_frames=3, variant=variant)
        return out


_mel("pwg")
_mel("tacotron")


def _resample_lengths(sr_in, sr_out):
    """The input lengths that give FD_RESAMPLE_TILE - 1 and + 1 outputs."""
    from fastdiff_amd import resample
    want, found = (_capi.FD_RESAMPLE_TILE - 1, _capi.FD_RESAMPLE_TILE + 1), []
    for w in want:
        found.append(next(n for n in range(1, 4096) if resample.out_len(n, sr_in, sr_out) == w))
    return found


def _resample(sr_in, sr_out, kind, offset):
    @case(f"resample-{sr_in}-{sr_out}-{kind}" + ("-off4" if offset else ""))
    def fn(g):
        m = model()
        lo, hi = _resample_lengths(sr_in, sr_out)
        out = {}
        for tag, valid in _ragged("", (lo // 2, lo, hi)):
            if kind == "s16x2":
                x = _padded((_wave(1, 3, hi * 2) * 32767).to(torch.int16).view(3, hi, 2), valid)
                out["y" + tag] = m.resample(g.tensor(x, offset), sr_in, sr_out, valid=valid, channels=2)
            else:
                out["y" + tag] = m.resample(g.tensor(_padded(_wave(1, 3, hi), valid), offset), sr_in, sr_out, valid=valid)
        return out


for _pair in ((48000, 22050), (22050, 48000)):
    _resample(*_pair, "s16x2", 0)
    _resample(*_pair, "f32", 0)
_resample(48000, 22050, "s16x2", 4)          # fd_resample promises any alignment: one placement 4 bytes off
_resample(22050, 48000, "f32", 4)


@case("loudness")
def _loudness(g, n=_capi.FD_LOUDNESS_TILE + 1):
    m = model()
    out = {}
    for tag, valid in _ragged("", (8820, _capi.FD_LOUDNESS_TILE, n)):          # one gating block; the tile; one sample into the second tile
        wav = g.tensor(_padded(_wave(1, 3, n), valid))
        out.update(as_tensors(m.loudness(wav, valid=valid), "measure" + tag + " "))
        y, rec = m.loudness_normalize(wav, -23.0, valid=valid, return_record=True)
        out["float" + tag] = y
        out.update(as_tensors(rec, "float" + tag + " "))
        out["int16" + tag] = m.loudness_normalize(wav, -23.0, valid=valid, out="int16")
    return out


@case("stoi")
def _stoi(g):
    m = model()
    out = {}
    for tag, valid in _ragged("", (256, 4097, 4225)):          # STEADY_LENGTHS: the shortest, and two around a border
        clean = _padded(_wave(1, 3, 4225), valid)
        deg = _padded(clean + _wave(2, 3, 4225, scale=0.05), valid)
        out.update(as_tensors(m.stoi(g.tensor(clean), g.tensor(deg), valid=valid, sample_rate=10000), tag + " "))
    return out


@case("pitch")
def _pitch(g, hop=256):
    import test_pitch as tp
    m = model()
    frames = (tp.TILE_FRAMES[1], tp.FT + 1, 2 * tp.FT + 3)          # one frame, one into the second tile, the longest of TILE_FRAMES
    n = frames[-1] * hop
    out = {}
    for tag, valid in _ragged("", [f * hop for f in frames]):
        t = torch.arange(n) / 22050.0
        clean = _padded((0.5 * torch.sin(2 * np.pi * 220.0 * t)).repeat(3, 1) + _wave(1, 3, n, scale=0.01), valid)
        deg = _padded(clean + _wave(2, 3, n, scale=0.05), valid)
        cw, dw = g.tensor(clean), g.tensor(deg)
        out.update(as_tensors(m.pitch(cw, dw, valid=valid), tag + " "))
        f0, aper = m.pitch_track(cw, valid=valid)
        out.update({"f0" + tag: f0, "aper" + tag: aper})
    return out


@case("spectral")
def _spectral(g):
    m = model()
    out = {}
    for tag, valid in _ragged("", (1024, 1025, 2049)):          # LENGTHS: the shortest, and its neighbours of two borders
        clean = _padded(_wave(1, 3, 2049), valid)
        deg = _padded(clean + _wave(2, 3, 2049, scale=0.05), valid)
        out.update(as_tensors(m.spectral(g.tensor(clean), g.tensor(deg), valid=valid), tag + " "))
    return out


def _amp(seed, B, T):
    return rnd(seed, B, 513, T).abs() + 0.01


def _griffin_lim(T):
    @case(f"griffin-lim-T{T}")
    def fn(g):
        m = model()
        out = {}
        for tag, lens in _ragged("", (2, max(2, T - 1), T)):
            amp = _amp(T, 3, T)
            for b, v in enumerate(lens):
                amp[b, :, v:] = 0
            wav, rec = m.griffin_lim(g.tensor(amp), lens=lens, n_iters=1, seed=5, return_record=True)
            out["wav" + tag] = wav
            out.update(as_tensors(rec, tag + " "))
        angles = g.tensor(rnd(9, 3, 513, T))
        out["wav-angles"] = m.griffin_lim(g.tensor(_amp(T, 3, T)), n_iters=1, angles=angles)
        return out


_griffin_lim(2)
_griffin_lim(5)


@case("mel-to-linear", {("fd_get_mel_filterbank", 1): HOST_BANK, ("fd_mel_to_linear", 4): HOST_PINV})
def _mel_to_linear(g):
    m = model()
    return {f"amp{T}-{v}": m.mel_to_linear(g.tensor(rnd(T, 3, 80, T) - 2.0), variant=v) for T in (1, 5, 33) for v in ("pwg", "tacotron")}


@case("mel-to-linear-nnls", {("fd_get_mel_filterbank", 1): HOST_BANK, ("fd_mel_to_linear_nnls", 5): HOST_BANK, ("fd_mel_to_linear_nnls", 6): HOST_PINV})
def _nnls(g):
    m = model()
    out = {}
    for tag, lens in _ragged("", (1, _capi.FD_NNLS_FRAME_TILE, _capi.FD_NNLS_FRAME_TILE + 1)):
        mel = rnd(1, 3, 80, lens[0] if tag.endswith("last") else lens[-1]) - 2.0
        amp, rec = m.mel_to_linear(g.tensor(mel), inversion="nnls", nnls_iters=8, lens=lens, return_record=True)
        out["amp" + tag] = amp
        out.update(as_tensors(rec, tag + " "))
    return out


@case("peak-normalize-int16")
def _peak(g, L=1000):
    from fastdiff_amd import lvc_op
    m = model()
    wav = g.tensor(rnd(1, 3, 1, L))
    out = {"plain": m.peak_normalize_int16(wav)}
    for tag, valid in _ragged("", (1, 513, L)):
        out["ragged" + tag] = m.peak_normalize_int16(g.tensor(_padded(rnd(2, 3, L), valid).view(3, 1, L)), valid=valid)
    lib, h = m._ready(wav.device)                      # the entry point without `valid`, which the wrapper reaches through its ragged twin
    pcm = torch.empty((3, L), device=wav.device, dtype=torch.int16)
    _capi.check(lib, h, lib.fd_peak_normalize_int16(h, wav.data_ptr(), 3, L, pcm.data_ptr(), lvc_op._stream(wav.device)), "fd_peak_normalize_int16")
    out["c-plain"] = pcm
    return out


# =====================================================================================================================================
# Inference
# =====================================================================================================================================
def _sample_mask(B, T, lens):
    """True on the samples sample() / forward() specify: behind lens[b] * 256 a row is unspecified (FastDiff.sample)."""
    mask = torch.zeros(B, 1, T * 256, dtype=torch.bool)
    for b in range(B):
        mask[b, :, : (T if lens is None else lens[b]) * 256] = True
    return mask


def _infer(B, T):
    import synth
    lens_sets = [("", None)] + ([] if B == 1 else [("-short-first", sorted(range(T, T - B, -1))), ("-short-last", sorted(range(T, T - B, -1))[::-1])])
    if B > 1:
        lens_sets[1][1][0] = 1          # (the shortest item: one frame)
        lens_sets[2][1][-1] = 1

    def inputs(g, lens):
        mel = torch.from_numpy(synth.synth_mel(3, B, T).copy())
        x = torch.from_numpy(synth.hash_normal(3, 1, B * T * 256).reshape(B, 1, T * 256).copy())
        for b, v in enumerate(lens or []):
            mel[b, :, v:] = 0
            x[b, :, v * 256:] = 0
        return g.tensor(mel), g.tensor(x)

    @case(f"forward-{B}x{T}")
    def fwd(g):
        m, out, masks = model(), {}, {}
        for tag, lens in lens_sets:
            mel, x = inputs(g, lens)
            steps = g.tensor(torch.full((B, 1), 7.4132))
            with torch.no_grad():
                out["eps" + tag] = m((x, mel, steps), lens=lens)
            masks["eps" + tag] = _sample_mask(B, T, lens)
        return out, masks

    @case(f"sample-{B}x{T}")
    def smp(g):
        m, out, masks = model(), {}, {}
        for tag, lens in lens_sets:
            mel, x = inputs(g, lens)
            z = torch.from_numpy(np.stack([synth.hash_normal(3, 2 + n, B * T * 256).reshape(B, 1, T * 256) for n in range(2)]))
            with torch.no_grad():
                out["injected" + tag] = m.sample(mel, rows2(), x_T=x, noise=g.tensor(z), lens=lens)
                out["device-noise" + tag] = m.sample(mel, rows2(), seed=7, lens=lens)
            masks["injected" + tag] = masks["device-noise" + tag] = _sample_mask(B, T, lens)
        return out, masks


_infer(1, 1)
_infer(2, 17)
_infer(3, 49)


@case("sample-exact-T-buffers")
def _t_bucket(g, B=2, T=17):
    """Option t_bucket = 0: the library's buffers are laid out for T itself, not for T rounded up to 32 frames."""
    import synth
    m = model()
    m.set_option("t_bucket", "0")
    try:
        with torch.no_grad():
            y = m.sample(g.tensor(torch.from_numpy(synth.synth_mel(3, B, T).copy())), rows2(), seed=7, return_sequence=True)
    finally:
        m.set_option("t_bucket", "32")
    return {f"x{k}": t for k, t in enumerate(y)}


@case("sample-span-window")
def _span(g, T=200):
    """One window of tests/test_long_form.py's utterances: frames [64, 96) of 200, from the whole mel and from the part that holds its halo."""
    import synth
    from fastdiff_amd import longform
    m = model()
    mel = torch.from_numpy(synth.synth_mel(8, 1, T).copy())
    H = longform.halo_frames(2)
    lo, hi = max(0, 64 - H), min(T, 96 + H)
    with torch.no_grad():
        whole = longform.sample_span(m, g.tensor(mel), 0, T, 64, 96, rows2(), seed=5, stream_id=7)
        part = longform.sample_span(m, g.tensor(mel[:, :, lo:hi].contiguous()), lo, T, 64, 96, rows2(), seed=5, stream_id=7)
    return {"whole": whole, "part": part}


@case("sample-spans")
def _spans(g):
    """fd_sample_spans: two utterances in one call; outputs the caller places (the header promises any alignment: one 4 bytes off); and a
    stream pool, whose mel reaches its ring through fd_mel_ring_append."""
    import synth
    from fastdiff_amd import longform
    m = model()
    mels = [g.tensor(torch.from_numpy(synth.synth_mel(8 + i, 1, T).copy())) for i, T in enumerate((40, 70))]
    with torch.no_grad():
        ys = m.sample_long_batch(mels, rows2(), seed=5, stream_ids=[3, 4])
        outs = [g.empty((1, 1, 40 * 256), torch.float32, 4), g.empty((1, 1, 32 * 256), torch.float32, 0)]
        longform.sample_spans(m, [{"mel": mels[0][0], "out": outs[0], "mel_first": 0, "mel_frames": 40, "utt_frames": 40, "t0": 0, "t1": 40, "stream_id": 3},
                                  {"mel": mels[1][0], "out": outs[1], "mel_first": 0, "mel_frames": 70, "utt_frames": 70, "t0": 32, "t1": 64, "stream_id": 4}],
                              rows2(), seed=5)
        pool = m.stream_pool(rows2(), seed=5, max_streams=2, max_feed_frames=64)
        s = pool.open(3)
        pool.feed(s, g.tensor(mels[0][:, :, :25]))
        pool.feed(s, g.tensor(mels[0][:, :, 25:]))
        pool.close(s)
        piece = pool.step()[s]
    return {"long0": ys[0], "long1": ys[1], "placed0": outs[0], "placed1": outs[1], "pool": piece, "arena": pool.arena}


# =====================================================================================================================================
# The test
# =====================================================================================================================================
def _run(name):
    if name not in REPORTS:
        try:
            REPORTS[name] = guarded.run_case(CASES[name][0], torch.device(DEV, torch.cuda.current_device()))
        except RuntimeError as e:
            if "illegal memory access" in str(e) or "HIP error" in str(e):      # the device is gone for this process: start nothing more on it
                pytest.exit(f"{name}: {e}", returncode=3)
            raise
    return REPORTS[name]


def test_a_guarded_tensor_is_aligned_like_a_plain_allocation():
    with guarded.guarded(guarded.FILLS[0], DEV) as g:
        for n, dtype in ((1, torch.float32), (37, torch.float32), (4097, torch.float32), (5, torch.int16), (3, torch.int64), (144, torch.uint8)):
            plain = g._orig["empty"](n, dtype=dtype, device=DEV)
            t = torch.empty(n, dtype=dtype, device=DEV)
            assert t.data_ptr() % guarded.GRANULE == plain.data_ptr() % guarded.GRANULE == 0, (n, dtype)
        assert g.check() == [] and len(g.blocks) == 6


def test_the_three_properties_see_a_wrong_operator_on_the_device():
    """The harness' own CPU tests (test_guarded_harness.py) on device memory, with torch operations standing in for a kernel: a store one
    element behind the output, a load one element behind the input, an element that is never written."""
    N = 37

    def wide(t):
        room = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
        return torch.as_strided(t, (N + 1,), (1,), t.storage_offset()) if room > N else None

    def op(fault):
        def fn(g):
            x = g.tensor(torch.arange(1.0, N + 1))
            out = torch.empty(N, device=x.device)
            out.copy_(2 * x)
            w = wide(out if fault == "store" else x)
            if fault == "store" and w is not None:
                w[N] = 7.0
            if fault == "load" and w is not None:
                out[N - 1] += 0 * w[N]
            if fault == "skip" and g.fill is not None:
                out[N - 1] = torch.empty(N, device=x.device)[N - 1]
            return {"out": out}
        return fn

    dev = torch.device(DEV, torch.cuda.current_device())
    rep = guarded.run_case(op("store"), dev)
    assert [bad[2:] for bad in rep.guard] == [((N,), ("behind", 2)), ((N,), ("behind", 0))] and not rep.poison and not rep.plain
    for fault in ("load", "skip"):
        rep = guarded.run_case(op(fault), dev)
        assert not rep.guard and rep.poison == [("out", 1, N - 1)], (fault, rep.guard, rep.poison)
    assert guarded.run_case(op(None), dev).clean()


@pytest.mark.parametrize("name", list(CASES))
def test_operator_in_guarded_memory(name):
    rep = _run(name)
    declared = CASES[name][1]
    print(f"{name}: {sum(rep.calls.values())} library calls in the two guarded runs: {dict(rep.calls)}")
    assert not rep.guard, f"(a) guard bytes changed (fill, block, shape, where): {rep.guard}"
    assert not rep.poison, f"(b) the two poisons disagree (tensor, elements, first): {rep.poison}"
    assert not rep.plain, f"(c) guarded and plain runs disagree (tensor, elements, first): {rep.plain}"
    assert set(rep.unguarded) == set(declared), f"(d) pointers outside guarded memory: {rep.unguarded}, declared: {sorted(declared)}"
    assert rep.calls, "the case called no entry point"


# entry points that take a pointer but no tensor of a caller's on the device, or that have a test of their own
EXEMPT = {
    "fd_ema_multi": "tests/test_param_ema.py puts canaries round its segments",
    "fd_set_weight": "weight accessor (host data)", "fd_get_weight_image": "weight accessor (host data)",
    "fd_set_mel_filterbank": "filter-bank accessor (host data)", "fd_get_mel_filterbank": "filter-bank accessor (host data)",
    "fd_read_tap": "tap accessor (host buffer)",
    "fd_set_noise_streams": "host array of stream ids", "fd_resample_taps": "host array of taps",
    "fd_pitch_lags": "host structure and two host integers",
}


def required_entry_points(lib):
    """The fd_* functions with a c_void_p between the handle and the stream, or an array of structures that hold one."""
    need = set()
    for name, fn in vars(lib).items():
        if not name.startswith("fd_") or getattr(fn, "argtypes", None) is None:
            continue
        for t in fn.argtypes[1:-1]:
            pointee = getattr(t, "_type_", None)
            if t is ct.c_void_p or (isinstance(pointee, type) and issubclass(pointee, ct.Structure) and pointee is not _capi.FdWeightRef and
                                    any(ft is ct.c_void_p for _, ft in pointee._fields_)):
                need.add(name)
    return need


def test_every_entry_point_that_takes_a_tensor_is_reached():
    """From the call log of the guarded runs (a case that has not run in this process is run here): a new entry point without a case
    fails."""
    lib = _capi.load()
    need = required_entry_points(lib)
    assert set(EXEMPT) <= need, f"stale exemptions: {sorted(set(EXEMPT) - need)}"
    assert len(need) >= 70 and {"fd_sample_spans", "fd_mel_ring_append", "fd_forward", "fd_adamw_multi"} <= need
    reached = set()
    for name in CASES:
        reached |= set(_run(name).calls)
    missing = need - set(EXEMPT) - reached
    assert not missing, f"entry points no case reaches: {sorted(missing)}"
