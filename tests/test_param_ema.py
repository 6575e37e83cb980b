"""An exponential moving average of the parameters on the device (fd_ema_multi, fastdiff_amd.ParamEMA, TrainStep(ema_decay=...)).

CPU: the entry point is declared, exported and bound, the ctypes mirrors have the header's sizes; the refusals of ParamEMA and
FastDiff.use_weights; the host twin of the decay schedule.
GPU, the kernel on raw tensors: after 1, 2 and 11 applied steps every shadow is BIT-EQUAL to e + w * (p - e) evaluated by three separate
torch float32 operations on the host, with w = float32(1 - decay_t) from the host twin; a call without a newly applied step changes no
byte; 64 floats of canary on each side of every shadow segment stay as they were.  Sizes one below, at and above the 4096-element
workgroup tile, 8 and 130 tensors (two 64-record chunk borders), shadows and parameters at offsets that are and are not multiples of
4 floats (the 16-byte body and the element-wise path).
GPU, end to end: replays against eager steps, against a TrainStep without the average, the warm-up's tracelessness, a skipped step,
a checkpoint round trip.

No tolerance anywhere: the kernel rounds operation by operation (the file's fp contract(off)), and the decision's double division is
IEEE on both sides.
"""
import ctypes as ct
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import synth    # noqa: E402

import fastdiff_amd                                   # noqa: E402
from fastdiff_amd import _capi, ema, schedules       # noqa: E402

SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 8195)
CANARY = 64
CANARY_VALUE = -12345.678
CHECK_AT = (1, 2, 11)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_train.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    assert "fd_ema_multi" in declared and "fd_ema_multi" in _capi.EXPORTS and hasattr(lib, "fd_ema_multi")
    for struct in ("fd_ema_item", "fd_ema_hyper", "fd_ema_state"):
        assert re.search(r"typedef struct %s\b" % struct, header), struct
    assert lib.fd_ema_multi(None, None, 0, None, None, None, None) == _capi.FD_ERR_INVALID
    from fastdiff_amd import lvc_op
    for name in ("ema_multi", "new_ema_state", "read_ema_state"):
        assert callable(getattr(lvc_op, name)), name
    assert "ParamEMA" in fastdiff_amd.__all__ and fastdiff_amd.ParamEMA is ema.ParamEMA
    for method in ("update", "set_decay", "state", "state_dict", "load_state_dict", "copy_to"):
        assert callable(getattr(fastdiff_amd.ParamEMA, method)), method
    import inspect
    sig = inspect.signature(fastdiff_amd.TrainStep.__init__).parameters
    assert list(sig)[:10] == ["self", "model", "diffusion_hyperparams", "lr", "betas", "eps", "weight_decay", "clip_grad_norm", "seed", "graph"]
    for name, default in (("ema_decay", None), ("ema_warmup", True)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is default
    sig = inspect.signature(fastdiff_amd.ParamEMA.__init__).parameters
    assert (sig["decay"].default, sig["warmup"].default) == (0.999, True)
    assert inspect.signature(fastdiff_amd.Validator.__init__).parameters["weights"].default is None


def test_struct_sizes_match_the_header():
    assert ct.sizeof(_capi.FdEmaState) == 24
    assert ct.sizeof(_capi.FdEmaHyper) == 16
    assert ct.sizeof(_capi.FdEmaItem) == 24
    assert _capi.FdEmaState.w.offset == 16 and _capi.FdEmaState.apply.offset == 20


def test_param_ema_refuses_a_cpu_module():
    with pytest.raises(RuntimeError, match="HIP device"):
        fastdiff_amd.ParamEMA(fastdiff_amd.FastDiff())
    with pytest.raises(RuntimeError, match="HIP device"):
        fastdiff_amd.TrainStep(fastdiff_amd.FastDiff(), schedules.training_hyperparams(), ema_decay=0.9)


def test_use_weights_refuses_wrong_names_and_shapes():
    m = fastdiff_amd.FastDiff()
    good = {k: torch.zeros_like(v) for k, v in m.state_dict().items()}
    assert m.use_weights(good) is None and m.weights_source is good and m._weights_dirty
    assert m.use_weights(None) is good and m.weights_source is None
    name = "fc_t1.bias"
    missing = {k: v for k, v in good.items() if k != name}
    with pytest.raises(ValueError, match=re.escape(name)):
        m.use_weights(missing)
    with pytest.raises(ValueError, match="no_such_tensor"):
        m.use_weights(dict(good, no_such_tensor=torch.zeros(1)))
    with pytest.raises(ValueError, match=re.escape(name)):
        m.use_weights(dict(good, **{name: torch.zeros(good[name].numel() + 1)}))
    with pytest.raises(ValueError):
        m.use_weights(3.0)
    assert m.weights_source is None, "a refused source leaves the recorded one alone"


def test_decay_schedule_twin():
    for decay in (0.999, 0.9999, 0.3):
        for n in (0, 1, 9, 8990, 8991, 10 ** 6):
            assert ema.decay_at(n, decay) == min(decay, (1 + n) / (10 + n)), (decay, n)
            assert ema.decay_at(n, decay, warmup=False) == decay
    # the ramp reaches 0.999 at 8990 updates (8991 / 9000) and stays capped from there on
    assert ema.decay_at(8989, 0.999) < 0.999 and ema.decay_at(8991, 0.999) == 0.999 and ema.decay_at(10 ** 6, 0.999) == 0.999
    assert ema.decay_at(0, 0.999) == 0.1


# ------------------------------------------------------------------------------------------------------------------ GPU: the kernel
@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


def _layout(n_tensors):
    """(sizes, parameter offsets, shadow offsets): segments with CANARY floats between them; every third shadow and every fifth
    parameter starts 1, 2 or 3 floats off a 16-byte border."""
    sizes = [SIZES[i % len(SIZES)] for i in range(n_tensors)]
    p_off, e_off, pa, ea = [], [], 0, 0
    for i, n in enumerate(sizes):
        ea = (ea + CANARY + 3) // 4 * 4 + (1 + i % 3 if i % 3 == 1 or i % 7 == 3 else 0)
        pa = (pa + 3) // 4 * 4 + (2 if i % 5 == 2 else 0)
        e_off.append(ea)
        p_off.append(pa)
        ea += n
        pa += n
    return sizes, p_off, e_off, pa, ea + CANARY


def _weight(updates, decay, warmup):
    return np.float32(1.0 - ema.decay_at(updates, decay, warmup))


def _host_step(e, p, w):
    """e + w * (p - e): three float32 operations, each rounded on its own."""
    d = p - e
    d = d * torch.tensor(w, dtype=torch.float32)
    return e + d


@pytest.mark.gpu
@pytest.mark.parametrize("n_tensors", [8, 130])
@pytest.mark.parametrize("decay,warmup", [(0.3, True), (0.999, False)], ids=["warmup", "plain"])
def test_the_kernel_is_bit_equal_to_three_torch_operations(n_tensors, decay, warmup):
    from fastdiff_amd import lvc_op
    sizes, p_off, e_off, p_len, e_len = _layout(n_tensors)
    assert any(o % 4 for o in e_off) and any(o % 4 for o in p_off) and any(a % 4 == 0 and b % 4 == 0 for a, b in zip(p_off, e_off))
    assert n_tensors <= 64 or n_tensors > 128
    gen = torch.Generator().manual_seed(1000 * n_tensors + int(warmup))
    ebuf_host = torch.full((e_len,), CANARY_VALUE)
    for n, o in zip(sizes, e_off):
        ebuf_host[o: o + n] = torch.randn(n, generator=gen)
    ebuf = ebuf_host.cuda()
    pbuf = torch.zeros(p_len, device="cuda")
    assert ebuf.data_ptr() % 16 == 0 and pbuf.data_ptr() % 16 == 0
    P = [pbuf[o: o + n] for n, o in zip(sizes, p_off)]
    E = [ebuf[o: o + n] for n, o in zip(sizes, e_off)]
    want = [ebuf_host[o: o + n].clone() for n, o in zip(sizes, e_off)]
    hyper = torch.tensor([decay, 1.0 if warmup else 0.0], dtype=torch.float64, device="cuda")
    state, est = lvc_op.new_train_state("cuda"), lvc_op.new_ema_state("cuda")
    items = list(zip(P, E))
    applied = 0
    for k in range(1, max(CHECK_AT) + 1):
        p_host = torch.randn(p_len, generator=gen)
        pbuf.copy_(p_host)
        applied += 1 + k % 2                      # (the counter may jump: what matters is that it went up)
        state[1] = applied
        lvc_op.ema_multi(items, hyper, state, est)
        w = _weight(k - 1, decay, warmup)
        want = [_host_step(e, p_host[o: o + n], w) for e, n, o in zip(want, sizes, p_off)]
        if k not in CHECK_AT:
            continue
        got = lvc_op.read_ema_state(est)
        assert (got["updates"], got["seen_applied"], got["apply"]) == (k, applied, 1), (k, got)
        assert np.float32(got["w"]) == w, (k, got["w"], w)
        host = ebuf.cpu()
        for i, (n, o) in enumerate(zip(sizes, e_off)):
            assert torch.equal(host[o: o + n].view(torch.int32), want[i].view(torch.int32)), \
                (k, i, n, o % 4, p_off[i] % 4, float((host[o: o + n] - want[i]).abs().max()))
        # a call without a newly applied step: no byte of the buffer moves, nothing is counted
        pbuf.copy_(torch.randn(p_len, generator=gen))
        lvc_op.ema_multi(items, hyper, state, est)
        again = lvc_op.read_ema_state(est)
        assert (again["updates"], again["seen_applied"], again["apply"]) == (k, applied, 0), (k, again)
        assert torch.equal(ebuf.cpu().view(torch.int32), host.view(torch.int32)), k
    # the canaries, and with them everything outside the segments
    mask = torch.ones(e_len, dtype=torch.bool)
    for n, o in zip(sizes, e_off):
        assert o >= CANARY
        mask[o: o + n] = False
    final = ebuf.cpu()
    assert mask.sum() >= CANARY * (n_tensors + 1)
    assert (final[mask] == np.float32(CANARY_VALUE)).all()
    assert lvc_op.read_train_state(state)["applied"] == applied, "the train state is only read"


@pytest.mark.gpu
def test_refused_calls():
    from fastdiff_amd import lvc_op
    lib, h = lvc_op._handle(torch.device("cuda", torch.cuda.current_device()))
    p, e = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    hyper = torch.tensor([0.9, 1.0], dtype=torch.float64, device="cuda")
    state, est = lvc_op.new_train_state("cuda"), lvc_op.new_ema_state("cuda")
    item = _capi.FdEmaItem(p.data_ptr(), e.data_ptr(), 8)
    ok = (ct.byref(item), 1, hyper.data_ptr(), state.data_ptr(), est.data_ptr())
    for i, bad in ((0, None), (1, 0), (2, None), (3, None), (4, None)):
        args = list(ok)
        args[i] = bad
        assert lib.fd_ema_multi(h, *args, None) == _capi.FD_ERR_INVALID, i
        assert b"fd_ema_multi" in lib.fd_last_error(h)
    for bad_item in (_capi.FdEmaItem(None, e.data_ptr(), 8), _capi.FdEmaItem(p.data_ptr(), None, 8), _capi.FdEmaItem(p.data_ptr(), e.data_ptr(), 0)):
        assert lib.fd_ema_multi(h, ct.byref(bad_item), 1, *ok[2:], None) == _capi.FD_ERR_INVALID
        assert b"item 0" in lib.fd_last_error(h)
    torch.cuda.synchronize()
    assert not e.any() and lvc_op.read_ema_state(est)["updates"] == 0


# ------------------------------------------------------------------------------------------------------------------ GPU: end to end
STEPS, DECAY, SEED = 5, 0.9, 1234


def _batch(gc, B=2, T=6):
    """The smallest module input tests/test_train_step.py trains on."""
    mel = torch.from_numpy(synth.synth_mel(3, B, T)).cuda()
    wav = (0.3 * gc.hash_normal_torch(3, 1, B * T * 256)).view(B, 1, T * 256)
    return mel, wav


def _bits(tensors):
    return [t.detach().clone().view(torch.int32) for t in tensors]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def runs(gc):
    """Five steps three ways from the same weights, seed and batch: replayed with the average, eager with the average, replayed
    without it.  What the graph run's shadow and record held when its first replay began is kept too."""
    dh = schedules.training_hyperparams()
    mel, wav = _batch(gc)
    out = {"dh": dh, "mel": mel, "wav": wav}
    first_replay = {}
    orig = torch.cuda.CUDAGraph.replay

    def replay(self):
        ts = first_replay.get("watch")
        if ts is not None and "shadow" not in first_replay:
            torch.cuda.synchronize()
            first_replay["shadow"] = _bits(ts.ema.tensors.values())
            first_replay["state"] = ts.ema.state()
            first_replay["params"] = _bits(ts.params)
        return orig(self)

    torch.cuda.CUDAGraph.replay = replay
    try:
        for tag, graph, decay in (("graph", True, DECAY), ("eager", False, DECAY), ("plain", True, None)):
            m = gc.make_model().train()
            p0 = _bits(m.state_dict().values())
            ts = fastdiff_amd.TrainStep(m, dh, seed=SEED, graph=graph, ema_decay=decay)
            if tag == "graph":
                first_replay["watch"] = ts
            for _ in range(STEPS):
                ts.step(mel, wav)
            first_replay.pop("watch", None)
            torch.cuda.synchronize()
            out[tag] = {"model": m, "ts": ts, "p0": p0, "params": _bits(m.state_dict().values()),
                        "shadow": None if decay is None else _bits(ts.ema.tensors.values())}
    finally:
        torch.cuda.CUDAGraph.replay = orig
    out["first_replay"] = first_replay
    return out


@pytest.mark.gpu
def test_replays_equal_eager_steps_and_leave_the_optimizer_alone(runs):
    g, e, plain = runs["graph"], runs["eager"], runs["plain"]
    assert g["ts"]._graph is not None and e["ts"]._graph is None and plain["ts"].ema is None
    assert _same(g["p0"], e["p0"]) and _same(g["p0"], plain["p0"])
    assert not _same(g["params"], g["p0"]), "five steps moved the parameters"
    assert _same(g["shadow"], e["shadow"])
    assert _same(g["params"], e["params"])
    assert _same(g["params"], plain["params"]), "the average does not touch the optimizer"
    for run in (g, e):
        assert run["ts"].state()["applied"] == STEPS
        assert run["ts"].ema.state() == {"updates": STEPS, "seen_applied": STEPS}
    assert not _same(g["shadow"], g["params"]) and not _same(g["shadow"], g["p0"])
    # the shadow's layout: state_dict() order, segments on multiples of 4 floats, weight_g and weight_v on their own
    avg = g["ts"].ema
    assert list(avg.tensors) == list(g["model"].state_dict())
    assert any(k.endswith("weight_g") for k in avg.tensors) and any(k.endswith("weight_v") for k in avg.tensors)
    assert all((t.data_ptr() - avg.shadow.data_ptr()) % 16 == 0 and t.shape == p.shape for t, p in zip(avg.tensors.values(), g["model"].state_dict().values()))


@pytest.mark.gpu
def test_warm_up_and_capture_leave_no_trace(runs):
    """When the first replay began -- after the constructor, three warm-up steps and the capture -- the shadow was the initial
    parameters bit for bit and its record empty; and the first update was therefore the schedule's first."""
    first = runs["first_replay"]
    assert _same(first["shadow"], runs["graph"]["p0"])
    assert _same(first["params"], runs["graph"]["p0"])
    assert first["state"] == {"updates": 0, "seen_applied": 0}
    m = runs["plain"]["model"]
    fresh = fastdiff_amd.ParamEMA(m)
    assert _same(_bits(fresh.tensors.values()), _bits(m.state_dict().values())) and fresh.state() == {"updates": 0, "seen_applied": 0}


@pytest.mark.gpu
def test_a_checkpoint_round_trip_continues_bit_equal(gc, runs):
    g = runs["graph"]
    ts, m = g["ts"], g["model"]
    sd = ts.state_dict()
    assert set(sd["ema"]) == {"decay", "warmup", "updates", "seen_applied", "shadow"} and sd["ema"]["updates"] == STEPS
    assert sd["ema"]["decay"] == DECAY and sd["ema"]["warmup"] is True and list(sd["ema"]["shadow"]) == list(m.state_dict())
    # torch's optimizer goes on ignoring what its layout has no place for
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros_like(p)) for p in m.parameters()], lr=1.0)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 2e-4
    other = fastdiff_amd.FastDiff()
    other.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    other = other.cuda().train()
    resumed = fastdiff_amd.TrainStep(other, runs["dh"], seed=SEED, graph=False, ema_decay=0.5, ema_warmup=False)
    resumed.load_state_dict(sd)
    assert resumed.ema.decay == DECAY and resumed.ema.warmup is True
    for _ in range(3):
        ts.step(runs["mel"], runs["wav"])
        resumed.step(runs["mel"], runs["wav"])
    torch.cuda.synchronize()
    assert ts.state()["applied"] == resumed.state()["applied"] == STEPS + 3
    assert ts.ema.state() == resumed.ema.state() == {"updates": STEPS + 3, "seen_applied": STEPS + 3}
    assert _same(_bits(m.state_dict().values()), _bits(other.state_dict().values()))
    assert _same(_bits(ts.ema.tensors.values()), _bits(resumed.ema.tensors.values()))
    # without an "ema" entry the average starts again from the parameters as loaded
    del sd["ema"]
    resumed.load_state_dict(sd)
    assert _same(_bits(resumed.ema.tensors.values()), _bits(other.state_dict().values()))
    assert resumed.ema.state() == {"updates": 0, "seen_applied": STEPS}
    # a shadow with other names or shapes is refused
    bad = ts.ema.state_dict()
    bad["shadow"].pop("fc_t1.bias")
    with pytest.raises(ValueError, match="names"):
        resumed.ema.load_state_dict(bad)
    bad = ts.ema.state_dict()
    bad["shadow"]["fc_t1.bias"] = bad["shadow"]["fc_t1.bias"][:-1]
    with pytest.raises(ValueError, match="fc_t1.bias"):
        resumed.ema.load_state_dict(bad)


@pytest.mark.gpu
def test_a_skipped_step_leaves_the_average_alone(runs):
    e = runs["eager"]
    ts = e["ts"]
    before_shadow, before_params = _bits(ts.ema.tensors.values()), _bits(ts.params)
    before = (ts.state(), ts.ema.state())
    wav = runs["wav"].clone()
    wav[0] = float("nan")
    ts.step(runs["mel"], wav)
    st = ts.state()
    assert (st["iter"], st["applied"], st["skipped"]) == (before[0]["iter"] + 1, before[0]["applied"], before[0]["skipped"] + 1), st
    assert ts.ema.state() == before[1]
    assert _same(_bits(ts.ema.tensors.values()), before_shadow) and _same(_bits(ts.params), before_params)
    # and the next good step moves it again, by the schedule's next weight
    ts.step(runs["mel"], runs["wav"])
    assert ts.ema.state() == {"updates": before[1]["updates"] + 1, "seen_applied": before[0]["applied"] + 1}
    w = _weight(before[1]["updates"], DECAY, True)
    want = [_host_step(s.view(torch.float32).cpu(), p.detach().cpu(), w) for s, p in zip(before_shadow, ts.ema.params)]
    got = [t.cpu() for t in ts.ema.tensors.values()]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))
    # set_decay reaches the device; copy_to writes the shadow over a module's parameters
    ts.ema.set_decay(0.25)
    assert float(ts.ema._hyper_dev[0]) == 0.25 and float(ts.ema._hyper_dev[1]) == 1.0
    target = runs["plain"]["model"]
    versions = [p._version for p in target.parameters()]
    ts.ema.copy_to(target)
    assert _same(_bits(target.state_dict().values()), _bits(ts.ema.tensors.values()))
    assert all(p._version > v for p, v in zip(target.parameters(), versions))
