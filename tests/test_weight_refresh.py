"""Inference weight packs refreshed on the device from live parameters (fd_refresh_weights_device, FastDiff.refresh_weights).

CPU: the entry points are declared, exported and bound; a NULL handle is refused; the layout functions that the host and the device
packer share (csrc/fd_wpack.h, read through fd_pack_source) agree with the loops they replaced, restated here, and invert
fd_kernel_index / fd_bias_index.
GPU: the refreshed weight image against a host commit of the same parameters, byte for byte (no tolerance: both sides are
deterministic and the fold's summation order is specified); results after a refresh against a fresh module that loaded the same
state_dict through the host; captured graphs survive a refresh; a weight that leaves the fp16 range drops them exactly once; the
validate-train-validate sequence with TrainStep; the fallbacks and the refused calls.
"""
import ctypes as ct
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

import fastdiff_amd
from fastdiff_amd import _capi, schedules

NEW = ("fd_refresh_weights_device", "fd_get_weight_image", "fd_get_weight_flags")
B, T, N = 1, 16, 3
UP = "lvc_blocks.1.upsample.weight"


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    for method in ("refresh_weights", "weight_image", "weight_flags"):
        assert callable(getattr(fastdiff_amd.FastDiff, method))
    assert lib.fd_refresh_weights_device(None, None, 0, None) == _capi.FD_ERR_INVALID
    assert lib.fd_refresh_weights_device(None, (_capi.FdWeightRef * 1)(), 1, None) == _capi.FD_ERR_INVALID


def _src(pack, p0, p1, pos):
    v = _capi.load().fd_pack_source(pack.encode(), p0, p1, int(pos))
    assert v >= 0, (pack, p0, p1, pos)
    return v


def test_shared_layout_functions_agree_with_the_loops_they_replaced():
    """Every map of csrc/fd_wpack.h against the nested loops of the host packer before it was moved there (restated below from the
    packs' documented layouts), on every position of the small packs and a spread of the large ones."""
    rng = np.random.default_rng(7)
    # fp32 A operands [mt][s4][lane][4], kk = 2*(4*s4+r) + (lane>>5) = tap*cin + ci
    for cout, cin, ks in ((32, 32, 3), (32, 32, 1), (64, 80, 5), (64, 64, 3)):
        ns4, n = cin * ks // 8, cout // 32 * (cin * ks // 8) * 256
        seen = set()
        for d in (range(n) if n <= 4096 else rng.choice(n, 2000, replace=False)):
            r, lane, q = d & 3, (d >> 2) & 63, d >> 8
            s4, mt = q % ns4, q // ns4
            o, kk = mt * 32 + (lane & 31), 2 * (4 * s4 + r) + (lane >> 5)
            want = (o * cin + kk % cin) * ks + kk // cin
            assert _src("pack_a", cin, ks, d) == want, (cout, cin, ks, d)
            seen.add(want)
        if n <= 4096:
            assert seen == set(range(cout * cin * ks))          # a permutation of the weight
        # fp16 pieces [mt][piece][kg][lane = out%32 + 32 g][8], k = 16 kg + 8 g + e
        inner = cin * ks // 16 * 512
        for pos in rng.choice(cout // 32 * inner, min(cout // 32 * inner, 1500), replace=False):
            mt, i = pos // inner, pos % inner
            row, k = (i >> 3) & 31, 16 * (i >> 9) + 8 * ((i >> 8) & 1) + (i & 7)
            assert _src("a_h2", cin, ks, pos) == ((mt * 32 + row) * cin + k % cin) * ks + k // cin, (cin, ks, pos)
    # ConvTranspose [in][out][2r] per phase: sel 0 the nearer input (tap kA), sel 1 the one before it (tap kA + r)
    for r in (8, 4):
        def tap(ph, sel, r=r):
            kA = ph + r // 2 if ph < r // 2 else ph - r // 2
            return kA + r if sel else kA
        for d in rng.choice(r * 2048, 1500, replace=False):
            q, lane, s4, ph = d & 3, (d >> 2) & 63, (d >> 8) & 7, d >> 11
            kk = 2 * (4 * s4 + q) + (lane >> 5)
            assert _src("up", r, 0, d) == ((kk & 31) * 32 + (lane & 31)) * 2 * r + tap(ph, kk >> 5), (r, d)
            ph, i = d // 2048, d % 2048
            row, k = (i >> 3) & 31, 16 * (i >> 9) + 8 * ((i >> 8) & 1) + (i & 7)
            assert _src("up_h2", r, 0, d) == ((k & 31) * 32 + row) * 2 * r + tap(ph, k >> 5), (r, d)
    # hop-8 tiles [rt][tap][piece][64 lane][8]: lane = out%16 + 16 g holds input channels 8g .. 8g+7
    seen = set()
    for pos in range(6 * 512):
        rt_tap, idx = pos // 512, pos % 512
        lane = idx >> 3
        want = ((16 * (rt_tap // 3) + (lane & 15)) * 32 + 8 * (lane >> 4) + (idx & 7)) * 3 + rt_tap % 3
        assert _src("h16", 0, 0, pos) == want
        seen.add(want)
    assert seen == set(range(32 * 32 * 3))
    # final_conv in register order [mt*2 + hi][8 r][8]: channel = 16 mt + 4 hi + (r & 3) + 8 (r >> 2); tap 7 is the pad
    for d in range(256):
        part, r, k = d >> 6, (d >> 3) & 7, d & 7
        want = 224 if k == 7 else (16 * (part >> 1) + 4 * (part & 1) + (r & 3) + 8 * (r >> 2)) * 7 + k
        assert _src("final_fuse", 0, 0, d) == want
    # the GEMM's tile positions: fp32 [24 s4][lane][4], fp16 [12 kg][lane][8]; k = tap*64 + channel, weight [64][3]
    for d in range(24 * 256):
        r, lane, s4 = d & 3, (d >> 2) & 63, d >> 8
        kk = 2 * (4 * s4 + r) + (lane >> 5)
        assert _src("gemm", 0, 0, d) == (lane & 31) * 192 + (kk % 64) * 3 + kk // 64
    for i in range(12 * 512):
        row, k = (i >> 3) & 31, 16 * (i >> 9) + 8 * ((i >> 8) & 1) + (i & 7)
        assert _src("gemm_h2", 0, 0, i) == row * 192 + (k % 64) * 3 + k // 64


def test_gemm_columns_invert_the_record_layout():
    """The row behind a packed column is the inverse of fd_kernel_index / fd_bias_index -- over the whole record."""
    lib = _capi.load()
    rows = np.array([_src("gemm_row", 0, 0, pp) for pp in range(24832)])
    assert sorted(rows) == list(range(24832))
    for layer in range(4):
        for o in range(64):
            assert rows[lib.fd_bias_index(layer, o)] == 24576 + layer * 64 + o
            for i in (0, 7, 13, 31):
                for k in range(3):
                    assert rows[lib.fd_kernel_index(layer, i, o, k)] == ((layer * 32 + i) * 64 + o) * 3 + k


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def sched():
    return load_golden("schedule")


def _perturbed_state(gc, seed=77):
    """The state_dict of module A: the synthetic weights with both weight-norm factors scaled row by row, so that folded rows span
    about 2^-30 .. 2^3, and the fp16 split's edge cases planted in a tensor that is not normed."""
    import synth
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(1234).items()}
    g = torch.Generator().manual_seed(seed)
    for k in sd:
        if k.endswith("weight_g"):
            rows = sd[k].shape[0]
            # g = 2^e (up to sign and a mantissa): folded |w| <= |g|, e in [-30, 3]
            e = torch.randint(-30, 4, (rows, 1, 1), generator=g).float()
            sd[k] = torch.sign(sd[k] + 1e-30) * (1.0 + torch.rand((rows, 1, 1), generator=g)) * torch.exp2(e - 1)
            v = k[:-1] + "v"
            sd[v] = sd[v] * torch.exp2(torch.randint(-6, 7, (rows, 1, 1), generator=g).float())
    up = sd[UP].view(-1)
    up[0], up[1] = 0.0, -0.0
    up[2] = 2.0 ** -15 * 1.3          # hi is an fp16 subnormal
    up[3] = 2.0 ** -26 * 1.7          # below half the smallest subnormal: hi = 0, all of it in lo
    up[4] = 1.0 + 2.0 ** -11          # an exact tie of the fp16 mantissa: to even, down
    up[5] = 1.0 + 3 * 2.0 ** -11      # ... and up
    up[6] = 2.0 - 2.0 ** -12          # rounds up across the binade, to 2.0
    up[7] = -(2.0 ** -14) * (1 - 2.0 ** -12)      # a subnormal that rounds up to the smallest normal
    return sd


def _module(sd, device="cuda"):
    m = fastdiff_amd.FastDiff()
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to(device).eval()


def _write_params(m, sd):
    """sd's values into m's parameters through raw storage: what an optimizer kernel does -- torch's version counters do not move."""
    with torch.no_grad():
        for k, t in m.state_dict().items():
            t.data.copy_(sd[k].to(t.device))      # (.data: a tensor with a version counter of its own)


def same(a, b):
    """Bit equality (a NaN equals itself)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _inputs(gc, sched):
    import synth
    mel = torch.from_numpy(synth.synth_mel(11, B, T)).cuda()
    rows, _ = gc.table_rows(sched, N)
    x_T = gc.hash_normal_torch(5, 1, B * T * 256).view(B, 1, T * 256)
    noise = torch.stack([gc.hash_normal_torch(5, 2 + n, B * T * 256).view(B, 1, T * 256) for n in range(N)])
    audio = 0.5 * gc.hash_normal_torch(5, 9, B * T * 256).view(B, 1, T * 256)
    steps = torch.tensor([[37.0]], device="cuda")
    return mel, rows, x_T, noise, audio, steps


@pytest.fixture(scope="module")
def host_A(gc, sched):
    """Module A committed through the host on a handle of its own: the reference of tests 1 and 2, computed once."""
    sd = _perturbed_state(gc)
    mel, rows, x_T, noise, audio, steps = _inputs(gc, sched)
    a = _module(sd)
    with torch.no_grad():
        y = a.sample(mel, rows, x_T=x_T, noise=noise).clone()
        f = a((audio, mel, steps)).clone()
    assert a.last_refresh.startswith("host")
    return dict(sd=sd, image=a.weight_image(), flags=a.weight_flags(), sample=y, forward=f)


@pytest.mark.gpu
def test_refreshed_image_and_results_equal_a_host_commit(gc, sched, host_A):
    """Tests 1 and 2 of the issue: handle 2 is committed with OTHER weights, samples once (a captured graph), is refreshed with A's
    parameters, and must then hold A's image byte for byte, the same flags, its graph, and compute what the host-committed A computes.  (That the graph
    is also REPLAYED after a refresh is test_graphs_survive_a_refresh's, on weights of ordinary size: A's rows of up to 2^3 can push an
    activation out of the fp16 range, and the call is then run again on fp32 kernels, which are graphs of their own.)"""
    mel, rows, x_T, noise, audio, steps = _inputs(gc, sched)
    m = gc.make_model(seed=4321)
    with torch.no_grad():
        y_other = m.sample(mel, rows, x_T=x_T, noise=noise).clone()
    resident = m.counter("graphs_resident")
    assert resident >= 1 and not same(y_other, host_A["sample"])
    sig = m._synced_state
    _write_params(m, host_A["sd"])
    assert m._state_signature() == sig, "the raw write must be invisible to the signature check, as an optimizer kernel's is"
    m.refresh_weights()
    image, flags = m.weight_image(), m.weight_flags()
    diff = np.flatnonzero(image != host_A["image"]) if image.shape == host_A["image"].shape else None
    if diff is not None and diff.size:      # where: the first runs of differing bytes (a gap of more than 64 equal bytes ends a run)
        cut = np.flatnonzero(np.diff(diff) > 64)[:8]
        print("differing runs:", [(int(a), int(b)) for a, b in zip(diff[np.r_[0, cut + 1]], diff[np.r_[cut, diff.size - 1]])])
    state = (m.counter("graphs_resident"), m.counter("refresh_graph_drops"))
    with torch.no_grad():
        y = m.sample(mel, rows, x_T=x_T, noise=noise)
        f = m((audio, mel, steps))
    print(f"last_refresh {m.last_refresh!r}; weight image: {image.size} bytes (host {host_A['image'].size}), "
          f"{'-' if diff is None else diff.size} differ" + (f", first at {diff[0]}, last at {diff[-1]}" if diff is not None and diff.size else "")
          + f"; flags {flags} (host {host_A['flags']}); graphs resident {state[0]} (before {resident}), dropped {state[1]}; "
          f"sample equal {same(y, host_A['sample'])}, forward equal {same(f, host_A['forward'])}; calls redone {m.counter('calls_redone')}")
    assert m.last_refresh == "device", m.last_refresh
    assert diff is not None and diff.size == 0
    assert flags == host_A["flags"] == 63
    assert state == (resident, 0)
    assert same(y, host_A["sample"])
    assert same(f, host_A["forward"])


@pytest.mark.gpu
def test_graphs_survive_a_refresh(gc, sched):
    """Test 3: sample, refresh to other weights, sample the same shape: a graph hit, no capture, the new weights' result."""
    import synth
    mel, rows, x_T, noise, _, _ = _inputs(gc, sched)
    new = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(99).items()}
    twin = _module(new)
    m = gc.make_model()
    with torch.no_grad():
        want = twin.sample(mel, rows, x_T=x_T, noise=noise)
        y0 = m.sample(mel, rows, x_T=x_T, noise=noise).clone()
        caps, hits = m.counter("graph_captures"), m.counter("graph_hits")
        assert caps >= 1
        _write_params(m, new)
        m.refresh_weights()
        y1 = m.sample(mel, rows, x_T=x_T, noise=noise)
    assert m.last_refresh == "device"
    assert m.counter("graph_captures") == caps and m.counter("graph_hits") > hits
    assert same(y1, want) and not same(y1, y0)


@pytest.mark.gpu
def test_a_weight_leaving_the_fp16_range_drops_the_graphs_once(gc, sched):
    """Test 4: one upsample weight at 40000 -- the ConvTranspose family's flag falls, like the host-committed twin's, the graphs are
    dropped exactly once, the result is the twin's; back in range, the flag returns (and the graphs are dropped once more: the
    family changes sides again)."""
    import synth
    mel, rows, x_T, noise, _, _ = _inputs(gc, sched)
    good = {k: torch.from_numpy(v.copy()) for k, v in synth.synth_state_dict(1234).items()}
    bad = {k: v.clone() for k, v in good.items()}
    bad[UP].view(-1)[17] = 40000.0
    twin = _module(bad)
    m = gc.make_model()
    with torch.no_grad():
        want = twin.sample(mel, rows, x_T=x_T, noise=noise)
        y_good = m.sample(mel, rows, x_T=x_T, noise=noise).clone()
        assert m.weight_flags() == 63 and twin.weight_flags() == 63 & ~16
        _write_params(m, bad)
        m.refresh_weights()
        got = m.sample(mel, rows, x_T=x_T, noise=noise)
        assert m.weight_flags() == twin.weight_flags()
        assert same(got, want)
        assert m.counter("refresh_graph_drops") == 1
        assert np.array_equal(m.weight_image(), twin.weight_image())
        again = m.sample(mel, rows, x_T=x_T, noise=noise)
        assert same(again, want) and m.counter("refresh_graph_drops") == 1
        _write_params(m, good)
        m.refresh_weights()
        assert m.weight_flags() == 63
        assert same(m.sample(mel, rows, x_T=x_T, noise=noise), y_good)
    assert m.counter("refresh_graph_drops") == 2 and m.last_refresh == "device"


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_validation_after_training_steps_sees_the_trained_weights(gc, graph):
    """Test 5, the staleness sequence: eval forward, two TrainStep steps, the same eval forward.  The second must differ from the first
    and be bit-equal to a fresh module loaded from the trained state_dict -- and the weights must have got there on the device."""
    import synth
    Bt, Tt = 2, 16
    mel = torch.from_numpy(synth.synth_mel(3, Bt, Tt)).cuda()
    wav = (0.3 * gc.hash_normal_torch(3, 1, Bt * Tt * 256)).view(Bt, 1, Tt * 256)
    audio = 0.5 * gc.hash_normal_torch(5, 9, Bt * Tt * 256).view(Bt, 1, Tt * 256)
    steps = torch.tensor([[37.0], [512.0]], device="cuda")
    m = gc.make_model().train()
    ts = fastdiff_amd.TrainStep(m, schedules.training_hyperparams(), lr=1e-2, graph=graph)

    def validate(net):
        net.eval()
        with torch.no_grad():
            y = net((audio, mel, steps)).clone()
        net.train()
        return y

    y0 = validate(m)
    for _ in range(2):
        ts.step(mel, wav)
    y1 = validate(m)
    assert m.last_refresh == "device", m.last_refresh
    st = ts.state()
    assert st["applied"] == 2, st
    fresh = _module({k: v.detach().cpu() for k, v in m.state_dict().items()})
    want = validate(fresh)
    assert torch.isfinite(y1).all()
    assert not same(y1, y0), "the weights moved (lr = 1e-2): the second validation must see them"
    assert same(y1, want)


@pytest.mark.gpu
def test_a_generic_architecture_refreshes_through_the_host(gc):
    """Test 6a: another architecture than base.yaml's has no device packer: refresh_weights() goes through the host, says so, and the
    module computes what a fresh twin of the new weights computes."""
    torch.manual_seed(3)
    kw = dict(upsample_ratios=[8, 8, 2, 2])
    g = fastdiff_amd.FastDiff(**kw).cuda().eval()
    Tg = 8
    mel = torch.randn(1, 80, Tg, device="cuda")
    audio = torch.randn(1, 1, Tg * 256, device="cuda")
    steps = torch.tensor([[5.0]], device="cuda")
    with torch.no_grad():
        y0 = g((audio, mel, steps)).clone()
        new = {k: v + 0.01 * torch.randn_like(v) for k, v in g.state_dict().items()}
        _write_params(g, new)
        g.refresh_weights()
        assert g.last_refresh.startswith("host: "), g.last_refresh
        y1 = g((audio, mel, steps))
        twin = fastdiff_amd.FastDiff(**kw)
        twin.load_state_dict({k: v.cpu() for k, v in new.items()})
        want = twin.cuda().eval()((audio, mel, steps))
    assert same(y1, want) and not same(y1, y0)


def _refs(sd, drop=None, reshape=None):
    names = [k.encode() for k in sd if k != drop]
    tensors = [sd[k.decode()] for k in names]
    shapes = [tuple(t.shape) if k.decode() != reshape else tuple(t.shape)[::-1] for k, t in zip(names, tensors)]
    dims = [(ct.c_int64 * len(s))(*s) for s in shapes]
    items = (_capi.FdWeightRef * len(names))(*[_capi.FdWeightRef(k, t.data_ptr(), ct.addressof(d), len(d), 0) for k, t, d in zip(names, tensors, dims)])
    return items, len(names), (names, dims)


@pytest.mark.gpu
def test_refused_calls_leave_the_weights_alone(gc):
    """Test 6b: no committed weights, a wrong shape, a missing tensor: the call's error, its text, and an unchanged weight image."""
    lib = _capi.load()
    m = gc.make_model()
    dev = torch.device("cuda", torch.cuda.current_device())
    sd = m.state_dict()
    stream = m._stream(dev)
    fresh = gc.make_model()
    lib_, = (fresh._ensure_handle(dev),)
    items, n, keep = _refs(sd)
    assert lib_.fd_refresh_weights_device(fresh._handle, items, n, stream) == _capi.FD_ERR_INVALID
    assert b"fd_commit_weights" in lib.fd_last_error(fresh._handle)
    m._ready(dev)
    before = m.weight_image()
    for kw, text in ((dict(reshape=UP), b"size mismatch"), (dict(drop="fc_t1.bias"), b"missing tensor fc_t1.bias")):
        items, n, keep = _refs(sd, **kw)
        assert lib.fd_refresh_weights_device(m._handle, items, n, stream) == _capi.FD_ERR_INVALID, kw
        assert text in lib.fd_last_error(m._handle), lib.fd_last_error(m._handle)
    torch.cuda.synchronize()
    assert np.array_equal(m.weight_image(), before)
    assert m.counter("weight_refreshes") == 0
