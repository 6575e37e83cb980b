"""Cases of the guarded-memory suite (tests/guarded_suite.py): the training operators with every gradient, the step, the scheduling network.
"""
import copy

import pytest
import torch

from guarded_suite import DEV, case, grads, leaf, rnd

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
