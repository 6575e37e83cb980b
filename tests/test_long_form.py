"""Long-form and streaming synthesis (fd_sample_span, FastDiff.sample_long / stream, infer --long_form).

CPU: the per-step halo the library uses is measured here on the float64 port of the network (oracle/torch_eager.py): perturbing one input
sample or one mel frame moves the outputs of one denoiser step only within h frames, and two reverse steps within 2h -- the cone a
window must keep away from its inner edges.  GPU: the windowed result equals the whole-utterance sampler bit for bit, past the length
the whole call refuses too, and a stream of chunks equals it as well."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

HOP = 256


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def _lib():
    from fastdiff_amd import _capi
    return _capi.load()


def test_halo_frames_is_linear_in_the_steps():
    lib = _lib()
    h = lib.fd_sample_halo_frames(1)
    assert h > 0
    for N in (1, 2, 3, 4, 6, 8, 200, 1000, 1024):
        assert lib.fd_sample_halo_frames(N) == N * h
    for N in (0, -1, 1025, 1 << 20):
        assert lib.fd_sample_halo_frames(N) < 0


def test_span_entry_points_are_exported():
    from fastdiff_amd import _capi
    lib = _lib()
    for name in ("fd_sample_halo_frames", "fd_sample_span"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fastdiff_hip_ext.h")).read()
    assert "FD_API int fd_sample_span(" in header and "FD_API int fd_sample_halo_frames(" in header


def _changed(d):
    nz = torch.nonzero(d > 0).flatten()
    assert nz.numel() > 0
    return int(nz.min()), int(nz.max())


def _reach(base, perturbed, at_sample=None, at_frame=None):
    """Samples by which the outputs that changed reach past the perturbed sample / the perturbed frame's samples."""
    lo, hi = _changed((perturbed - base).abs())
    if at_sample is not None:
        return max(at_sample - lo, hi - at_sample)
    return max(at_frame * HOP - lo, hi - (at_frame * HOP + HOP - 1))


@pytest.fixture(scope="module")
def eager64():
    import synth
    from torch_eager import EagerFastDiff
    T = 96
    m = EagerFastDiff(synth.synth_state_dict(1234), dtype=torch.float64)
    x = torch.from_numpy(synth.hash_normal(5, 1, T * HOP).reshape(1, 1, T * HOP)).double()
    mel = torch.from_numpy(synth.synth_mel(5, 1, T)).double()
    return m, x, mel, T


def test_halo_covers_the_measured_reach_of_one_step(eager64):
    """One denoiser forward at T = 96 frames: one input sample perturbed at eight phases inside its frame (the down path samples by
    4, 32, 256), one mel frame perturbed; the halo of one step covers the farthest change and is at most one frame above it."""
    m, x, mel, T = eager64
    h = _lib().fd_sample_halo_frames(1)
    f = T // 2
    phases = (0, 1, 37, 100, 128, 200, 254, 255)
    xs = x.repeat(len(phases) + 2, 1, 1)
    for i, ph in enumerate(phases):
        xs[i + 1, 0, f * HOP + ph] += 1.0
    mels = mel.repeat(len(phases) + 2, 1, 1)
    mels[-1, :, f] += 1.0
    with torch.no_grad():
        y = m.forward(xs, mels, torch.full((xs.shape[0],), 7.4132, dtype=torch.float64))[:, 0]
    audio = max(_reach(y[0], y[i + 1], at_sample=f * HOP + ph) for i, ph in enumerate(phases))
    cond = _reach(y[0], y[-1], at_frame=f)
    reach = max(audio, cond)
    print(f"one step: input-sample reach {audio}, mel-frame reach {cond} samples; halo {h} frames = {h * HOP} samples")
    assert 0 < reach <= h * HOP
    assert h <= -(-reach // HOP) + 1


def test_halo_cone_grows_additively_over_steps(eager64):
    """Two reverse steps (DDPM update): the change of one x_T sample or one mel frame spreads past one step's halo but stays within
    fd_sample_halo_frames(2) = 2 h frames -- the cone of N steps is N h."""
    m, x, mel, T = eager64
    lib = _lib()
    h1, h2 = lib.fd_sample_halo_frames(1), lib.fd_sample_halo_frames(2)
    rows = load_golden("schedule")
    n4 = {k: rows[f"N4_{k}"] for k in ("steps", "c_eps", "c_div", "sigma_hat")}
    table = [{"t": float(np.float32(n4["steps"][n])), "c_eps": float(n4["c_eps"][n]), "c_div": float(n4["c_div"][n]),
              "sigma": float(n4["sigma_hat"][n]), "add_noise": 1} for n in (3, 2)]
    f = T // 2
    p = f * HOP + 100
    xs = x.repeat(3, 1, 1)
    xs[1, 0, p] += 1.0
    mels = mel.repeat(3, 1, 1)
    mels[2, :, f] += 1.0
    import synth
    z = torch.from_numpy(np.stack([synth.hash_normal(6, 2 + k, T * HOP) for k in range(2)])).double().reshape(2, 1, 1, T * HOP).repeat(1, 3, 1, 1)
    with torch.no_grad():
        y = m.sample(mels, table, xs, noise=z)[:, 0]
    audio, cond = _reach(y[0], y[1], at_sample=p), _reach(y[0], y[2], at_frame=f)
    print(f"two steps: input-sample reach {audio}, mel-frame reach {cond} samples; halo {h2} frames")
    assert max(audio, cond) <= h2 * HOP
    assert max(audio, cond) > h1 * HOP          # one step's halo would not do


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gc():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def model(gc):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gc.make_model()


@pytest.fixture(scope="module")
def sched():
    return load_golden("schedule")


def _mel(seed, T):
    import synth
    return torch.from_numpy(synth.synth_mel(seed, 1, T)).cuda()


def _whole(model, mel, rows, ddim=False, seed=0, sid=0, **kw):
    return model.sample(mel, rows, ddim=ddim, seed=seed, stream_ids=[sid], **kw)


def _no_handover(model, redone_before):
    assert model.counter("calls_redone") == redone_before
    assert model.counter("pieces_redone") == 0
    assert not model.read_tap("range_flags_call").view(np.int32).any()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [3, 4, 6, 8])
def test_sample_long_equals_the_whole_utterance(model, gc, sched, N):
    """sample_long == sample(..., stream_ids=[sid]) bit for bit, DDPM and "ddim", T in {200, 864, 2017, 6912}, windows of 32, 64, 256
    centre frames and the default; no window batch handed a stage over to the fp32 kernels."""
    rows, _ = gc.table_rows(sched, N)
    with torch.no_grad():
        for ddim in (False, True):
            for T in (200, 864, 2017, 6912):
                mel = _mel(T % 97 + N, T)
                sid = 1000 + T
                ref = _whole(model, mel, rows, ddim=ddim, seed=5, sid=sid)
                redone = model.counter("calls_redone")
                for wf in (32, 64, 256, None):
                    y = model.sample_long(mel, rows, ddim=ddim, seed=5, stream_id=sid, window_frames=wf)
                    assert y.shape == ref.shape
                    assert torch.equal(y, ref), (N, ddim, T, wf, float((y - ref).abs().max()))
                    _no_handover(model, redone)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [{"gemm": "fp32", "lvc": "fp32", "conv": "fp32"}, {"graph": "0"}, {"hoist": "on"}, {"hoist": "off"}],
                         ids=["fp32", "graph0", "hoist_on", "hoist_off"])
def test_sample_long_equals_the_whole_utterance_under_options(gc, sched, opts):
    m = gc.make_model()
    for k, v in opts.items():
        m.set_option(k, v)
    rows, _ = gc.table_rows(sched, 4)
    mel = _mel(8, 2017)
    with torch.no_grad():
        ref = _whole(m, mel, rows, seed=3, sid=7)
        for wf in (64, None):
            y = m.sample_long(mel, rows, seed=3, stream_id=7, window_frames=wf)
            assert torch.equal(y, ref), (opts, wf)


@pytest.mark.gpu
def test_sample_long_n200(model, gc):
    from fastdiff_amd import infer
    rows = infer._step_rows(model, 200, None, None)
    T = 8000
    mel = _mel(9, T)
    with torch.no_grad():
        ref = _whole(model, mel, rows, seed=11, sid=3)
        redone = model.counter("calls_redone")
        y = model.sample_long(mel, rows, seed=11, stream_id=3)
    assert torch.equal(y, ref)
    _no_handover(model, redone)


@pytest.mark.gpu
def test_sample_long_with_injected_noise(model, gc, sched):
    import synth
    N, T = 4, 2017
    rows, _ = gc.table_rows(sched, N)
    mel = _mel(12, T)
    x_T = torch.from_numpy(synth.hash_normal(12, 1, T * HOP).reshape(1, 1, T * HOP)).cuda()
    z = torch.from_numpy(gc.exec_order_noise(gc.noise_from_seed(12, 1, T, N))).cuda()
    with torch.no_grad():
        ref = model.sample(mel, rows, x_T=x_T, noise=z)
        for wf in (32, 256, None):
            assert torch.equal(model.sample_long(mel, rows, x_T=x_T, noise=z, window_frames=wf), ref), wf
        ref = model.sample(mel, rows, ddim=True, x_T=x_T, noise=z)
        assert torch.equal(model.sample_long(mel, rows, ddim=True, x_T=x_T, noise=z, window_frames=64), ref)


@pytest.mark.gpu
def test_past_the_whole_call_limit(gc, sched):
    """300,000 frames (about 58 minutes at 22.05 kHz): sample() refuses, sample_long computes it.  Three regions equal the centre of a
    plain sample() call on a 20k-frame sub-utterance cut out with H frames of margin (none at the utterance's own edges), fed the
    matching slices of mel, x_T and z -- an independent check of the cone argument through the existing entry point.  The device
    memory after 50k frames is the memory after 300k frames."""
    N = 4
    m = gc.make_model()
    rows, _ = gc.table_rows(sched, N)
    H = m.halo_frames(N)

    def inputs(T, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        mel = (torch.rand((1, 80, T), device="cuda", generator=g) * 5.0 - 5.0)
        x_T = torch.randn((1, 1, T * HOP), device="cuda", generator=g)
        z = torch.randn((N, 1, 1, T * HOP), device="cuda", generator=g)
        return mel, x_T, z

    with torch.no_grad():
        mel, x_T, z = inputs(50_000, 1)
        y = m.sample_long(mel, rows, x_T=x_T, noise=z)
        assert torch.isfinite(y).all()
        ws_50k = m.counter("workspace_bytes")
        del mel, x_T, z, y
        T = 300_000
        mel, x_T, z = inputs(T, 2)
        with pytest.raises(AssertionError, match="too large"):
            m.sample(mel, rows, x_T=x_T, noise=z)
        y = m.sample_long(mel, rows, x_T=x_T, noise=z)
        assert m.counter("workspace_bytes") == ws_50k
        assert y.shape == (1, 1, T * HOP) and torch.isfinite(y).all()
        S = 20_000
        for a in (0, 150_016, T - S):
            lo, hi = max(0, a - H), min(T, a + S + H)
            assert lo % 32 == 0
            sub = m.sample(mel[:, :, lo:hi].contiguous(), rows, x_T=x_T[:, :, lo * HOP:hi * HOP].contiguous(),
                           noise=z[..., lo * HOP:hi * HOP].contiguous())
            assert torch.equal(y[..., a * HOP:(a + S) * HOP], sub[..., (a - lo) * HOP:(a - lo + S) * HOP]), a


@pytest.mark.gpu
def test_stream_equals_sample_long(model, gc, sched):
    """Mel pushed in random chunks of 1..300 frames: the concatenated pieces equal sample_long bit for bit, and after every push
    all frames below F - H - chunk_frames + 1 have been returned."""
    N, T = 4, 3001
    rows, _ = gc.table_rows(sched, N)
    H = model.halo_frames(N)
    mel = _mel(13, T)
    rng = np.random.default_rng(2024)
    with torch.no_grad():
        ref = model.sample_long(mel, rows, seed=21, stream_id=5)
        s = model.stream(rows, seed=21, stream_id=5)
        pieces, F, got = [], 0, 0
        while F < T:
            t = int(min(T - F, rng.integers(1, 301)))
            chunk = mel[0, :, F:F + t] if rng.integers(2) else mel[:, :, F:F + t]
            y = s.push(chunk)
            F += t
            got += y.numel()
            pieces.append(y)
            assert got % HOP == 0 and got // HOP >= F - H - 32 + 1, (F, got // HOP)
            assert s.mel.shape[-1] < 2 * H + 32        # only the frames still needed are kept
        pieces.append(s.close())
    assert torch.equal(torch.cat(pieces), ref.reshape(-1))


@pytest.mark.gpu
def test_windowed_against_float64_oracle(model, gc, sched, oracle64):
    """T = 864, N = 4, 64-frame windows, injected x_T and z: the bar of the whole-utterance sampler test (1e-4)."""
    import synth
    T, N = 864, 4
    mel = synth.synth_mel(21, 1, T)
    x_T = synth.hash_normal(21, 1, T * HOP).reshape(1, 1, T * HOP)
    z = gc.noise_from_seed(21, 1, T, N)
    rows, table = gc.table_rows(sched, N)
    ref = oracle64.sample(mel, table, x_T, z)
    with torch.no_grad():
        y = model.sample_long(torch.from_numpy(mel).cuda(), rows, x_T=torch.from_numpy(x_T).cuda(),
                              noise=torch.from_numpy(gc.exec_order_noise(z)).cuda(), window_frames=64)
    d = gc.maxdiff(y.cpu().numpy(), ref)
    print(f"windowed N=4 T=864: max|d| = {d:.3e}")
    assert d < 1e-4


@pytest.mark.gpu
def test_span_refusals(model, gc, sched):
    from fastdiff_amd import longform
    rows, _ = gc.table_rows(sched, 4)
    H = model.halo_frames(4)
    T = 400
    mel = _mel(3, T)
    with torch.no_grad():
        for t0, t1 in ((16, 128), (0, 100), (0, T + 32)):           # misaligned t0, misaligned t1 (not the end), t1 past the utterance
            with pytest.raises(AssertionError):
                longform.sample_span(model, mel, 0, T, t0, t1, rows)
        with pytest.raises(AssertionError, match="need mel"):         # mel starts inside the halo of t0
            longform.sample_span(model, mel[:, :, 100:].contiguous(), 100, T, 128, 256, rows)
        with pytest.raises(AssertionError, match="need mel"):         # streaming: t1 + H past the mel
            longform.sample_span(model, mel, 0, -1, 0, 352, rows)
        from fastdiff_amd import infer
        rows200 = infer._step_rows(model, 200, None, None)
        with pytest.raises(AssertionError, match="N <= 8"):
            model.sample_long(mel[:, :, :64].contiguous(), rows200, noise=torch.zeros((200, 1, 1, 64 * HOP), device="cuda"))
        with pytest.raises(AssertionError):
            longform.halo_frames(0)
        model.set_option("kernels.lvc", "naive")
        try:
            with pytest.raises(NotImplementedError, match="naive"):
                model.sample_long(mel, rows)
        finally:
            model.set_option("kernels", "fast")
        import fastdiff_amd
        g = fastdiff_amd.FastDiff(upsample_ratios=[8, 8, 2, 2]).cuda().eval()
        with pytest.raises(NotImplementedError, match="architecture"):
            g.sample_long(mel, rows)


@pytest.mark.gpu
def test_infer_long_form_writes_the_same_wavs(tmp_path):
    import synth
    from fastdiff_amd import infer
    src = tmp_path / "mels"
    src.mkdir()
    for i, T in enumerate((200, 333, 517, 700, 864)):
        np.save(src / f"utt{i}.npy", np.ascontiguousarray(synth.synth_mel(40 + i, 1, T)[0].T))
    infer.main(["--test_input_dir", str(src), "--out_dir", str(tmp_path / "a")])
    infer.main(["--test_input_dir", str(src), "--out_dir", str(tmp_path / "b"), "--long_form"])
    names = sorted(os.listdir(tmp_path / "a"))
    assert len(names) == 5 and names == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes(), n
