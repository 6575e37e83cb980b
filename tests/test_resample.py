"""Sample-rate conversion on the device (fd_resample, fastdiff_amd/resample.py, FastDiff.resample) and what is built on it:
infer.load_wav_inputs for recordings of any rate and channel count, infer.synthesize(out_sample_rate=...), TrainCorpus.from_wav_dir.

CPU: the entry points are declared, exported and bound; fd_resample_out_len; the filter design against scipy.signal.firwin (an
independent implementation) and the library's float32 taps against it; the operator's definition against scipy.signal.resample_poly;
the filter's pass band and stop band through the float64 host twin.
GPU: the kernel against the float64 sum over the SAME float32 taps and float32 inputs at its tile borders, with the derived bound
    |y - y64| <= K 2^-23 sum_k |h_k x_k|
(a float32 sum of K products obeys K 2^-24 sum |h_k x_k| to first order in any order, with or without FMA; twice that is asserted, per
output, and an output whose bound is 0 must be exactly 0); impulses at both edges; sample types and channels; ragged batches and
layouts, bit for bit; the three paths above end to end.
"""
import os
import re

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import TrainCorpus, _capi, infer, schedules
from fastdiff_amd import resample as rs

NEW = ("fd_resample_out_len", "fd_resample_taps", "fd_resample")
TILE = _capi.FD_RESAMPLE_TILE
# 147/320, 441/320, 1/2, 2/1, 320/441, 160/441
RATIOS = ((48000, 22050), (16000, 22050), (44100, 22050), (22050, 44100), (22050, 16000), (22050, 8000))
# 20/441: K = 2823 taps, a tile needs 8.4k inputs -- more than one staging piece of the kernel (4096 samples)
LONG_SPAN = (22050, 1000)
_TAPS = {}


def taps_of(pair):
    if pair not in _TAPS:
        _TAPS[pair] = rs.taps(*pair)
    return _TAPS[pair]


def reference(x32, pair):
    """(y64, bound): the float64 sum over the library's float32 taps and the float32 inputs, and sum_k |h_k x_k| per output."""
    h = taps_of(pair)[0]
    x = np.asarray(x32, np.float32)
    return rs.resample_host(x, *pair, h=h), rs.resample_host(np.abs(x), *pair, h=np.abs(h))


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define\s+FD_RESAMPLE_TILE\s+(\d+)", header).group(1)) == _capi.FD_RESAMPLE_TILE
    assert callable(fastdiff_amd.FastDiff.resample) and callable(TrainCorpus.from_wav_dir)
    assert "resample" in fastdiff_amd.__all__ and fastdiff_amd.resample is rs
    assert lib.fd_resample(None, None, 0, 1, 1, 1, 1, None, 48000, 22050, None, 1, None) == _capi.FD_ERR_INVALID
    assert lib.fd_resample_taps(0, 22050, None, 0, None, None, None) == _capi.FD_ERR_INVALID
    assert lib.fd_resample_taps(22050, 22051, None, 0, None, None, None) == _capi.FD_ERR_UNSUPPORTED


def test_out_len():
    lib = _capi.load()
    for sr_in, sr_out in RATIOS[:3] + ((24000, 22050), (22050, 16000), (22050, 48000), (22050, 44100), (22050, 8000), (96000, 22050)):
        up, down, _, _ = rs.ratio(sr_in, sr_out)
        for n in (1, 2, 255, 256, 257, 10 ** 9):
            assert lib.fd_resample_out_len(n, sr_in, sr_out) == -(-n * up // down) == rs.out_len(n, sr_in, sr_out), (n, sr_in, sr_out)
    assert lib.fd_resample_out_len(100, 22050, 22051) == _capi.FD_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        rs.out_len(100, 22050, 22051)
    for n in (0, 1, 257, 10 ** 9):
        assert lib.fd_resample_out_len(n, 22050, 22050) == n == lib.fd_resample_out_len(n, 7, 7)
    assert lib.fd_resample_out_len(-1, 48000, 22050) == _capi.FD_ERR_INVALID


@pytest.mark.parametrize("pair", RATIOS + ((96000, 22050), (22050, 48000), (24000, 22050)))
def test_design_against_scipy_firwin(pair):
    up, down, half, K = rs.ratio(*pair)
    q = max(up, down)
    g_scipy = signal.firwin(2 * half + 1, rs.ROLLOFF / q, window=("kaiser", rs.BETA))
    g = rs.design(*pair)
    assert g.dtype == np.float64 and g.shape == g_scipy.shape
    d = np.abs(g - g_scipy).max() / np.abs(g_scipy).max()
    print(f"{pair}: |g - g_scipy| / max|g| = {d:.2e}")
    assert d <= 1e-12
    h32, u, dn, hf = taps_of(pair)
    assert (u, dn, hf) == (up, down, half) and h32.dtype == np.float32 and h32.shape == g.shape and K == -(-(2 * half + 1) // up)
    ref = up * g_scipy
    excess = np.abs(h32.astype(np.float64) - ref) - (2.0 ** -24 * np.abs(ref) + 1e-12 * up * np.abs(g_scipy).max())
    assert excess.max() <= 0.0, excess.max()


def test_taps_per_output_of_the_documented_conversions():
    assert [rs.ratio(a, 22050)[3] for a in (48000, 16000, 96000)] == [279, 129, 558]


@pytest.mark.parametrize("pair", RATIOS)
def test_definition_against_resample_poly(pair):
    h32, up, down, _ = taps_of(pair)
    rng = np.random.default_rng(up * 1000 + down)
    for n in (500, 777, 1000):
        x = rng.standard_normal(n)
        y = rs.resample_host(x, *pair, h=h32)
        y_poly = signal.resample_poly(x, up, down, window=h32.astype(np.float64) / up)
        assert y.shape == y_poly.shape == (-(-n * up // down),)
        assert np.abs(y - y_poly).max() <= 1e-12


def _tone(pair, f):
    """max |y - the same sine at the output rate| over the middle half of half a second, through the float64 twin"""
    sr_in, sr_out = pair
    x = np.sin(2 * np.pi * f * np.arange(sr_in // 2) / sr_in)
    y = rs.resample_host(x, sr_in, sr_out)
    t = np.arange(y.shape[0])
    mid = slice(y.shape[0] // 4, 3 * y.shape[0] // 4)
    want = np.sin(2 * np.pi * f * t / sr_out) if f < sr_out / 2 else np.zeros(y.shape[0])
    return np.abs(y - want)[mid].max()


@pytest.mark.parametrize("pair,f,bound", [((48000, 22050), 5000, 1e-7), ((22050, 48000), 5000, 1e-7), ((16000, 22050), 7000, 1e-6),
                                          ((48000, 22050), 12500, 1e-7), ((48000, 22050), 15000, 1e-7)])
def test_pass_band_and_stop_band_of_the_design(pair, f, bound):
    d = _tone(pair, f)
    print(f"{pair} {f} Hz: {d:.2e}")
    assert d <= bound


# ------------------------------------------------------------------------------------------------------------------ GPU
def lengths_for(pair):
    """Input lengths whose n_out is 1, TILE - 1, TILE, TILE + 1 and 2 TILE + 3 -- where the ratio cannot give a target exactly (an
    up-sampler's n_out moves in steps of up / down), the two lengths around it -- plus n_in = 1 and K - 1."""
    up, down, _, K = rs.ratio(*pair)
    ns = {1, K - 1}
    for m in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
        hi = (m - 1) * down // up + 1                    # the shortest input with n_out >= m
        assert rs.out_len(hi, *pair) >= m and (hi == 1 or rs.out_len(hi - 1, *pair) < m)
        ns.add(hi)
        if rs.out_len(hi, *pair) > m and hi > 1:
            ns.add(hi - 1)                               # ... and the longest with n_out < m
    return sorted(ns)


def test_lengths_reach_the_tile_borders():
    for pair in RATIOS + (LONG_SPAN,):
        outs = {rs.out_len(n, *pair) for n in lengths_for(pair)}
        up, down, _, _ = rs.ratio(*pair)
        for m in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3):
            around = any(o > m for o in outs) and (m == 1 or any(o < m for o in outs))
            assert m in outs or (up > down and around), (pair, m, sorted(outs))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", RATIOS + (LONG_SPAN,))
def test_kernel_against_float64_at_the_tile_borders(pair):
    up, down, half, K = rs.ratio(*pair)
    rng = np.random.default_rng(up * 7 + down)
    worst = 0.0
    for n in lengths_for(pair):
        x = rng.standard_normal(n).astype(np.float32)
        y64, bound = reference(x, pair)
        y = rs.resample(torch.from_numpy(x).cuda(), *pair)
        assert y.shape == (1, rs.out_len(n, *pair)) and y.dtype == torch.float32
        y = y[0].cpu().numpy().astype(np.float64)
        tol = K * 2.0 ** -23 * bound
        err = np.abs(y - y64)
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), (pair, n, int(np.argmax(err - tol)), float((err - tol).max()))
        assert not y[bound == 0.0].any()
    print(f"{pair}: K = {K}, worst |y - y64| / bound = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("pair", RATIOS)
def test_an_impulse_at_either_edge_returns_its_column_of_taps(pair):
    n = 700
    for at in (0, n - 1):
        x = np.zeros(n, np.float32)
        x[at] = 1.0
        y64, _ = reference(x, pair)                      # every output is one tap times 1 (or 0): exactly a float32
        y = rs.resample(torch.from_numpy(x).cuda(), *pair)[0].cpu().numpy()
        assert np.array_equal(y.astype(np.float64), y64), (pair, at)
        assert np.count_nonzero(y) > 0


def _raw(rng, dtype, n, C):
    if dtype == np.float32:
        return (rng.random((n, C)) * 2 - 1).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=(n, C), endpoint=True, dtype=dtype)


def _host_mono(raw):
    """pcm_to_float per sample, then the down-mix as an explicit float32 loop in channel order and one division"""
    f = infer.pcm_to_float(raw)
    s = f[:, 0].copy()
    for c in range(1, f.shape[1]):
        s = (s + f[:, c]).astype(np.float32)
    return s if f.shape[1] == 1 else (s / np.float32(f.shape[1])).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.uint8, np.float32])
def test_sample_types_and_channels_are_converted_in_the_kernel(dtype):
    rng = np.random.default_rng(5)
    pair, n = (16000, 22050), 613
    for C in (1, 2, 3):
        raw = _raw(rng, dtype, n, C)
        mono = _host_mono(raw)
        assert mono.dtype == np.float32
        want = rs.resample(torch.from_numpy(mono).cuda(), *pair)
        dev = torch.from_numpy(raw).cuda()
        got = rs.resample(dev if C > 1 else dev[:, 0].contiguous(), *pair, channels=C)
        assert torch.equal(got, want), (dtype, C)
    # equal rates: conversion and down-mix only
    raw = _raw(rng, np.int16, n, 2)
    same = rs.resample(torch.from_numpy(raw).cuda(), 22050, 22050, channels=2)
    assert same.shape == (1, n) and torch.equal(same[0].cpu(), torch.from_numpy(_host_mono(raw)))


@pytest.mark.gpu
def test_ragged_batches_and_layouts_leave_every_bit_alone():
    pair, n = (48000, 22050), 1301                       # three tiles of outputs
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((3, n)).astype(np.float32)).cuda()
    valid = (n, n - 1, 1)
    y = rs.resample(x, *pair, valid=valid)
    assert y.shape == (3, rs.out_len(n, *pair))
    alone = [rs.resample(x[b, :v].clone(), *pair)[0] for b, v in enumerate(valid)]
    for b, v in enumerate(valid):
        m = rs.out_len(v, *pair)
        assert torch.equal(y[b, :m], alone[b]) and not y[b, m:].any(), b
    # the same rows 4 bytes off a 16-byte border, at a pitch that is no multiple of 4
    pitch = n + 2
    assert pitch % 4 != 0
    buf = torch.full((1 + 3 * pitch,), 1.0e3, device="cuda")
    rows = buf[1:].view(3, pitch)[:, :n]
    rows.copy_(x)
    assert rows.data_ptr() % 16 == 4 and rows.stride(0) == pitch
    assert torch.equal(rs.resample(rows, *pair, valid=valid), y)
    assert torch.equal(rs.resample(rows[1:2], *pair, valid=valid[1:2])[0, : rs.out_len(n - 1, *pair)], alone[1])
    # more items than one launch carries lengths for
    pair, n, B = (22050, 16000), 40, 2 * 64 + 2
    xb = torch.from_numpy(np.random.default_rng(10).standard_normal((B, n)).astype(np.float32)).cuda()
    vb = [1 + (7 * b) % n for b in range(B)]
    yb = rs.resample(xb, *pair, valid=vb)
    for b in (0, 63, 64, 65, 127, 128, B - 1):
        m = rs.out_len(vb[b], *pair)
        assert torch.equal(yb[b, :m], rs.resample(xb[b, : vb[b]].clone(), *pair)[0]) and not yb[b, m:].any(), b


@pytest.mark.gpu
def test_refusals_leave_a_message():
    x = torch.zeros(100, device="cuda")
    with pytest.raises(AssertionError, match="valid_in"):
        rs.resample(x, 48000, 22050, valid=[101])
    with pytest.raises(AssertionError, match="valid_in"):
        rs.resample(x, 48000, 22050, valid=[0])
    with pytest.raises(NotImplementedError):
        rs.resample(x, 22050, 22051)
    with pytest.raises(ValueError):
        rs.resample(x.double(), 48000, 22050)
    with pytest.raises(ValueError):
        rs.resample(x.view(50, 2), 48000, 22050, channels=3)
    lib = _capi.load()
    from fastdiff_amd import lvc_op
    _, h = lvc_op._handle(x.device)
    y = torch.zeros(46, device="cuda")
    assert rs.out_len(100, 48000, 22050) == 46
    assert lib.fd_resample(h, x.data_ptr(), 0, 9, 1, 100, 900, None, 48000, 22050, y.data_ptr(), 46, None) == _capi.FD_ERR_INVALID
    assert b"channels" in lib.fd_last_error(h)
    assert lib.fd_resample(h, x.data_ptr(), 0, 1, 1, 100, 100, None, 48000, 22050, y.data_ptr(), 45, None) == _capi.FD_ERR_INVALID
    assert b"dst_pitch" in lib.fd_last_error(h)
    assert lib.fd_resample(h, None, 0, 1, 1, 100, 100, None, 48000, 22050, y.data_ptr(), 46, None) == _capi.FD_ERR_INVALID
    assert b"null" in lib.fd_last_error(h)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_a_first_call_inside_a_capture_is_refused_and_a_later_one_replays():
    """fastdiff_hip_ext.h: a ratio's table is made at its first use, never inside a stream capture."""
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no table of any ratio yet
    lib, h = m._ready(torch.device("cuda"))
    pair, n = (48000, 22050), 64
    n_out = rs.out_len(n, *pair)
    rng = np.random.default_rng(21)
    xa, xb = (torch.from_numpy(rng.standard_normal((1, n)).astype(np.float32)).cuda() for _ in range(2))
    x, y = xa.clone(), torch.zeros((1, n_out), device="cuda")

    def call():
        return lib.fd_resample(h, x.data_ptr(), _capi.FD_PCM_F32, 1, 1, n, n, None, *pair, y.data_ptr(), n_out, m._stream(x.device))

    torch.cuda.synchronize()
    first = torch.cuda.CUDAGraph()
    with torch.cuda.graph(first):
        x.mul_(1.0)                                        # (so that the capture is not empty)
        rc = call()
        msg = lib.fd_last_error(h)
    assert rc == _capi.FD_ERR_STATE and b"stream capture" in msg, (rc, msg)
    torch.cuda.synchronize()
    want_a, want_b = m.resample(xa, *pair), m.resample(xb, *pair)      # outside: the table
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _capi.check(lib, h, call(), "fd_resample")
    for src, want in ((xa, want_a), (xb, want_b)):
        x.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert want.shape == y.shape and torch.equal(y, want)


@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def _speechlike(rng, n, C=None):
    t = np.arange(n)
    x = 0.4 * np.sin(2 * np.pi * t / 97.0) + 0.2 * np.sin(2 * np.pi * t / 13.7) + 0.05 * rng.standard_normal(n)
    if C is not None:
        x = np.stack([x * (0.9 - 0.2 * c) + 0.01 * rng.standard_normal(n) for c in range(C)], axis=1)
    return np.round(x * 20000).astype(np.int16)


@pytest.mark.gpu
def test_load_wav_inputs_takes_any_rate_and_channel_count(model, tmp_path):
    rng = np.random.default_rng(21)
    stereo48, mono16, mono22 = _speechlike(rng, 19200, 2), _speechlike(rng, 6400), _speechlike(rng, 8820)
    wavfile.write(tmp_path / "a48.wav", 48000, stereo48)
    wavfile.write(tmp_path / "b16.wav", 16000, mono16)
    wavfile.write(tmp_path / "c22.wav", 22050, mono22)
    items = infer.load_wav_inputs(model, str(tmp_path))
    assert [it["item_name"] for it in items] == ["a48.wav", "b16.wav", "c22.wav"]
    for it, raw, sr, C in ((items[0], stereo48, 48000, 2), (items[1], mono16, 16000, 1)):
        wav = model.resample(torch.from_numpy(raw).cuda(), sr, 22050, channels=C)
        want = model.mel_spectrogram(wav)[0].transpose(0, 1).contiguous().cpu()
        assert it["len"] == it["mel"].shape[0] == 1 + rs.out_len(raw.shape[0], sr, 22050) // 256
        assert torch.equal(it["mel"], want), it["item_name"]
    # a mono recording at the model's rate: the path of before, restated
    direct = model.mel_spectrogram(torch.from_numpy(infer.pcm_to_float(mono22)).cuda())[0].transpose(0, 1).contiguous().cpu()
    assert torch.equal(items[2]["mel"], direct) and items[2]["len"] == 1 + 8820 // 256
    for sr in (22050, 16000):                            # a sample type nobody defined a scale for is still refused, on either path
        with pytest.raises(ValueError, match="unsupported sample type"):
            infer.wav_to_device(model, np.zeros(64, np.int64), sr)


@pytest.mark.gpu
def test_synthesize_at_another_output_rate(model):
    rng = np.random.default_rng(4)
    items = [{"item_name": f"u{i}", "mel": torch.from_numpy((rng.random((t + 1, 80)) * 7.5 - 6.0).astype(np.float32)), "len": t + 1}
             for i, t in enumerate((5, 8))]
    plain = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=11)
    none = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=11, out_sample_rate=None)
    assert all(np.array_equal(plain[k], none[k]) and plain[k].tobytes() == none[k].tobytes() for k in plain)
    out = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=11, out_sample_rate=16000)
    assert {k: v.shape[0] for k, v in out.items()} == {"u0": rs.out_len(5 * 256, 22050, 16000), "u1": rs.out_len(8 * 256, 22050, 16000)}
    # the float waveform of the same micro-batch (longest first: u1, u0), then per item alone: resample first, normalise second
    mels, lens, names = infer.collate_test_batch([items[1], items[0]])
    assert names == ["u1", "u0"] and lens == [8, 5]
    rows = infer._step_rows(model, 4, None, None)
    with torch.no_grad():
        wav = model.sample(mels.cuda(), rows, ddim=False, seed=11, lens=lens, stream_ids=[1, 0])
    for b, (name, t) in enumerate(zip(names, lens)):
        own = model.resample(wav[b, 0, : t * 256].clone(), 22050, 16000)
        want = model.peak_normalize_int16(own.unsqueeze(1))[0].cpu().numpy()
        assert out[name].dtype == np.int16 and np.array_equal(out[name], want), name
        assert np.abs(out[name]).max() == 32767
    on_dev = infer.synthesize(model, [dict(it, mel=it["mel"].cuda()) for it in items], n_steps=4, max_batch=2, seed=11, out_sample_rate=16000,
                              return_device=True)
    assert all(np.array_equal(on_dev[k].cpu().numpy(), out[k]) for k in out)


@pytest.mark.gpu
def test_train_corpus_from_a_directory_of_recordings(tmp_path):
    import gpu_common
    rng = np.random.default_rng(33)
    model = gpu_common.make_model()
    recs = {"a.wav": _speechlike(rng, 4000), "b_short.wav": _speechlike(rng, 2000), "c.wav": _speechlike(rng, 5000, 2)}
    for name, pcm in recs.items():
        wavfile.write(tmp_path / name, 24000, pcm)
    corpus = TrainCorpus.from_wav_dir(model, str(tmp_path), max_samples=2560)
    # T = 1 + n' // 256 with n' = ceil(n 147 / 160): 15, 8 and 18 frames; kept when T > 2560 // 256
    assert [1 + rs.out_len(n, 24000, 22050) // 256 for n in (4000, 2000, 5000)] == [15, 8, 18]
    assert corpus.lengths.tolist() == [15, 18] and corpus.n_skipped == 1 and corpus.kept.tolist() == [0, 2] and corpus.n_items == 2
    assert corpus.frames == 10 and corpus.hop_size == 256 and corpus.frame_off_host.tolist() == [0, 15, 33] and corpus.wav.is_cuda
    wavs, mels = [], []
    for name in ("a.wav", "c.wav"):
        raw = torch.from_numpy(recs[name]).cuda()
        wav = model.resample(raw, 24000, 22050, channels=1 if raw.dim() == 1 else 2)[0]
        mel = model.mel_spectrogram(wav)[0]
        T = mel.shape[1]
        assert T == 1 + wav.shape[0] // 256
        mels.append(mel.transpose(0, 1))
        wavs.append(torch.cat([wav, torch.zeros(T * 256 - wav.shape[0], device="cuda")])[: T * 256])
    assert torch.equal(corpus.wav, torch.cat(wavs)) and torch.equal(corpus.mel, torch.cat(mels))
    ts = fastdiff_amd.TrainStep(model.train(), schedules.training_hyperparams(), seed=3, graph=False, corpus=corpus, batch_size=2)
    loss = ts.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


@pytest.mark.gpu
def test_the_cli_takes_mixed_recordings_and_writes_another_rate(tmp_path):
    """`python -m fastdiff_amd.infer --from_wav --out_sample_rate 48000` on a directory that mixes 16 / 22.05 / 24 / 48 kHz, mono and
    stereo (its main(), in this process)."""
    rng = np.random.default_rng(8)
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    frames = {}
    for name, sr, n, C in (("a16", 16000, 2400, None), ("b22", 22050, 3000, None), ("c24", 24000, 3300, 2), ("d48", 48000, 7000, 2)):
        wavfile.write(src / f"{name}.wav", sr, _speechlike(rng, n, C))
        frames[name] = rs.out_len(n, sr, 22050) // 256          # 1 + n' // 256 mel frames, the last one dropped by the collater
    infer.main(["--test_input_dir", str(src), "--from_wav", "--out_dir", str(out), "--N", "4", "--max_batch", "3", "--out_sample_rate", "48000"])
    for name, t in frames.items():
        sr, pcm = wavfile.read(out / f"{name}.wav_pred.wav")
        assert sr == 48000 and pcm.dtype == np.int16 and pcm.shape == (rs.out_len(t * 256, 22050, 48000),), name
        assert np.abs(pcm).max() == 32767
