"""BS.1770 loudness on the device (fd_loudness_design / _blocks / _measure / _normalize, FastDiff.loudness / loudness_normalize,
infer.synthesize(loudness=...), infer.load_wav_inputs(loud_norm=True), TrainCorpus.from_wav_dir(loud_norm=True)) against the float64
oracle tests/loudness_ref.py: pyloudnorm's meter restated in numpy + scipy.signal.lfilter, itself anchored on EBU Tech 3341's 997 Hz
sine.

Bounds.  lufs: 1e-4 LU (state, sums and the oracle are float64; an int16 LSB at full scale is 2.65e-4 LU, so the PCM bound needs it).
peak, blocks, gated, status: equal.  int16 output: +-1 of the oracle's (int16)(float32(wav) float32(gain) 32767f) (the gain may differ
in its last float32 bit); float32 output: 2 ulp.  SHORT / SILENT / CLIPPED rows: equal to the peak epilogue.  An utterance alone, in a
ragged batch with garbage behind it, and from call to call: the same bits.  The inputs keep every block at least 1e-3 LU away from
either gate (asserted on the oracle), so gate decisions cannot differ by rounding.
"""
import functools
import os
import re
import warnings

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import ROOT

import fastdiff_amd
from fastdiff_amd import TrainCorpus, _capi, infer
from fastdiff_amd import loudness as ld
import loudness_ref as ref

NEW = ("fd_loudness_design", "fd_loudness_blocks", "fd_loudness_measure", "fd_loudness_normalize")
TILE = _capi.FD_LOUDNESS_TILE
RATES = (22050, 16000, 48000)
SIGNALS = ("noise", "gated", "dclf")
TARGET = -23.0


def lengths_for(rate):
    return (int(0.4 * rate), int(0.4 * rate) + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + int(0.1 * rate) + 7, 3 * TILE + 4321)


@functools.lru_cache(maxsize=None)
def signal_of(kind, rate, n):
    """float32 [n] from a fixed seed.  noise: 0.1 N(0, 1); gated: a third 0.3 N, a third 0.003 N, the rest exact zeros (both gates act);
    dclf: 0.5 + 0.4 sin(2 pi 20 t) + 0.01 N (lives on the 38 Hz poles and on the carry between tiles); quiet: 1e-5 N (below -70 LUFS)."""
    rng = np.random.default_rng([SIGNALS.index(kind) if kind in SIGNALS else 9, rate, n])
    g = rng.standard_normal(n)
    if kind == "noise":
        x = 0.1 * g
    elif kind == "gated":
        x = np.zeros(n)
        x[: n // 3] = 0.3 * g[: n // 3]
        x[n // 3: 2 * (n // 3)] = 0.003 * g[n // 3: 2 * (n // 3)]
    elif kind == "dclf":
        x = 0.5 + 0.4 * np.sin(2 * np.pi * 20.0 * np.arange(n) / rate) + 0.01 * g
    else:
        x = 1e-5 * g
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(kind, rate, n, out=None):
    """The oracle's record of signal_of(kind, rate, n) (out None), or (output, record) normalised to TARGET; computed once, shared."""
    x = signal_of(kind, rate, n)
    return ref.measure(x, rate) if out is None else ref.normalize(x, rate, TARGET, out)


def ulp_diff(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fastdiff_hip_ext.h")).read()
    declared = set(re.findall(r"FD_API\s+[\w\s\*]+?\b(fd_\w+)\s*\(", header))
    lib = _capi.load()
    for name in NEW:
        assert name in declared and name in _capi.EXPORTS and hasattr(lib, name), name
    assert int(re.search(r"#define\s+FD_LOUDNESS_TILE\s+(\d+)", header).group(1)) == _capi.FD_LOUDNESS_TILE == ld.TILE
    assert ld.RECORD.itemsize == 32
    assert callable(fastdiff_amd.FastDiff.loudness) and callable(fastdiff_amd.FastDiff.loudness_normalize)
    assert "loudness" in fastdiff_amd.__all__ and fastdiff_amd.loudness is ld
    assert (ld.OK, ld.SHORT, ld.SILENT, ld.CLIPPED) == (ref.OK, ref.SHORT, ref.SILENT, ref.CLIPPED)
    assert lib.fd_loudness_measure(None, None, 1, 1, None, 22050, None, None) == _capi.FD_ERR_INVALID
    assert lib.fd_loudness_design(22050, None) == _capi.FD_ERR_INVALID
    assert lib.fd_loudness_design(7999, np.zeros(10).ctypes.data) == _capi.FD_ERR_INVALID
    assert lib.fd_loudness_blocks(-1, 22050) == _capi.FD_ERR_INVALID and lib.fd_loudness_blocks(100, 192001) == _capi.FD_ERR_INVALID


@pytest.mark.parametrize("rate", (48000, 22050, 16000))
def test_oracle_reads_the_997_hz_sine_of_ebu_tech_3341(rate):
    """Anchored outside this project: a full-scale 997 Hz sine reads -3.01 LUFS on a BS.1770 meter, +-0.1 LU being EBU Tech 3341's
    meter tolerance (pyloudnorm's filters put it at -3.05 / -3.07 / -3.08); scaling by g moves the reading by 20 log10 g."""
    x = np.sin(2 * np.pi * 997.0 * np.arange(5 * rate) / rate)
    r = ref.measure(x, rate)
    assert r["status"] == ref.OK and abs(r["lufs"] - (-3.01)) <= 0.1, r
    x32 = x.astype(np.float32)
    base = ref.measure(x32, rate)["lufs"]
    for g in (0.5, 0.125):                                 # exact in float32: the signal is scaled, not re-rounded
        assert abs(ref.measure(x32 * np.float32(g), rate)["lufs"] - (base + 20 * np.log10(g))) <= 1e-9


@pytest.mark.parametrize("rate", RATES + (24000, 44100))
def test_filter_design_equals_the_oracle(rate):
    got, want = ld.design(rate), ref.coef10(rate)
    assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want)), (got, want)


@pytest.mark.parametrize("rate", RATES + (24000, 44100))
def test_block_count_equals_the_oracle(rate):
    lo, hi = int(0.4 * rate) - 2, int(0.4 * rate) + 3 * int(0.1 * rate) + 2
    assert [ld.blocks(n, rate) for n in range(lo, hi + 1)] == [ref.blocks(n, rate) for n in range(lo, hi + 1)]
    if rate == 22050:
        assert [ld.blocks(n, rate) for n in (8819, 8820, 11025)] == [0, 1, 2]


def test_inputs_stay_clear_of_the_gates_and_take_every_branch():
    """A condition on the test's inputs, checked on the oracle: no block within 1e-3 LU of a threshold; the gated signal loses blocks
    at both gates; dc+lf at TARGET would clip."""
    for rate in RATES:
        for n in lengths_for(rate):
            for kind in SIGNALS:
                assert oracle(kind, rate, n)["margin"] >= 1e-3, (kind, rate, n)
            if n < int(0.4 * rate):                        # 48 kHz: a tile is shorter than one block -- these lengths are SHORT
                assert rate == 48000 and oracle("noise", rate, n)["status"] == ref.SHORT
                continue
            _, r = oracle("dclf", rate, n, "int16")
            assert r["status"] == ref.CLIPPED and 1.0 < float(r["peak"]) * 10.0 ** ((TARGET - r["lufs"]) / 20.0) < 1.2, (rate, n, r)
            assert oracle("noise", rate, n, "int16")[1]["status"] == ref.OK
        n = lengths_for(rate)[5]
        r = oracle("gated", rate, n)
        z = ref.block_powers(signal_of("gated", rate, n), rate)
        with np.errstate(divide="ignore"):
            absolute = int((-0.691 + 10 * np.log10(z) >= -70.0).sum())
        assert r["blocks"] >= absolute > r["gated"] > 0, (rate, r, absolute)
        assert rate == 48000 or r["blocks"] > absolute, (rate, r, absolute)      # (at 48 kHz every block still holds some of the 0.003 N)
    r = oracle("gated", 22050, lengths_for(22050)[5])
    assert (r["blocks"], r["gated"]) == (13, 6)
    assert oracle("quiet", 22050, TILE)["status"] == ref.SILENT


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    import gpu_common
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return gpu_common.make_model()


def _check_record(got, b, want, where):
    assert int(got["status"][b]) == want["status"], (where, got["status"][b], want)
    assert int(got["blocks"][b]) == want["blocks"] and int(got["gated"][b]) == want["gated"], (where, got["blocks"][b], got["gated"][b], want)
    assert got["peak"][b].tobytes() == np.float32(want["peak"]).tobytes(), (where, got["peak"][b], want["peak"])
    if want["status"] in (ref.OK, ref.CLIPPED):
        err = abs(float(got["lufs"][b]) - want["lufs"])
        print(f"{where}: lufs {got['lufs'][b]:.6f} oracle {want['lufs']:.6f} |diff| {err:.2e}")
        assert err <= 1e-4, (where, got["lufs"][b], want["lufs"])
    else:
        assert got["lufs"][b] == -np.inf, (where, got["lufs"][b])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("rate", RATES)
def test_measure_against_the_oracle_at_the_tile_borders(model, rate, kind):
    for n in lengths_for(rate):
        x = torch.from_numpy(signal_of(kind, rate, n).copy()).cuda()
        got = model.loudness(x, sample_rate=rate)
        _check_record(got, 0, oracle(kind, rate, n), (kind, rate, n))
        assert got["gain"][0] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_silent_and_short_utterances_get_their_status(model, rate):
    n = int(0.4 * rate)
    L = TILE + n + 5                                        # more than one tile and, at any rate, more than one block
    got = model.loudness(torch.zeros(2, L, device="cuda"), sample_rate=rate)
    assert list(got["status"]) == [ld.SILENT] * 2 and list(got["blocks"]) == [ref.blocks(L, rate)] * 2 and list(got["gated"]) == [0, 0]
    assert np.all(got["lufs"] == -np.inf) and np.all(got["peak"] == 0.0)
    x = signal_of("noise", rate, n)
    got = model.loudness(torch.from_numpy(x[: n - 1].copy()).cuda(), sample_rate=rate)
    assert int(got["status"][0]) == ld.SHORT and int(got["blocks"][0]) == 0 and got["lufs"][0] == -np.inf
    assert got["peak"][0].tobytes() == np.abs(x[: n - 1]).max().tobytes()
    _check_record(model.loudness(torch.from_numpy(signal_of("quiet", rate, L).copy()).cuda(), sample_rate=rate), 0, oracle("quiet", rate, L),
                  ("quiet", rate))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SIGNALS)
@pytest.mark.parametrize("rate", RATES)
def test_normalize_against_the_oracle(model, rate, kind):
    for n in lengths_for(rate):
        x = torch.from_numpy(signal_of(kind, rate, n).copy()).cuda()
        want16, r = oracle(kind, rate, n, "int16")
        want32, _ = oracle(kind, rate, n, "float")
        pcm, rec = model.loudness_normalize(x, TARGET, sample_rate=rate, out="int16", return_record=True)
        _check_record(rec, 0, r, (kind, rate, n))
        y = model.loudness_normalize(x, TARGET, sample_rate=rate, out="float")
        assert pcm.shape == (1, n) and pcm.dtype == torch.int16 and y.shape == (n,) and y.dtype == torch.float32
        d16 = np.abs(pcm[0].cpu().numpy().astype(np.int32) - want16.astype(np.int32)).max()
        d32 = ulp_diff(y.cpu().numpy(), want32).max()
        print(f"{kind} {rate} {n}: status {ld.STATUS[r['status']]} gain {rec['gain'][0]:.7f} oracle {r['gain']:.7f} int16 diff {d16} float ulp {d32:.2f}")
        assert d16 <= 1 and d32 <= 2.0, (kind, rate, n, d16, d32)
        if r["status"] != ref.OK:
            assert torch.equal(pcm, model.peak_normalize_int16(x.reshape(1, 1, n), valid=[n])), (kind, rate, n)
        else:
            assert abs(float(rec["gain"][0]) / float(r["gain"]) - 1.0) <= 2.0 ** -22


@pytest.mark.gpu
def test_utterances_that_cannot_be_scaled_fall_back_to_the_peak_epilogue(model):
    rate, L = 22050, TILE + 9
    rows = [signal_of("dclf", rate, L), signal_of("quiet", rate, L), signal_of("noise", rate, L), signal_of("noise", rate, L)]
    valid = [L, L, 8819, L]
    x = torch.from_numpy(np.stack(rows)).cuda()
    pcm, rec = model.loudness_normalize(x, TARGET, valid=valid, sample_rate=rate, out="int16", return_record=True)
    assert list(rec["status"]) == [ld.CLIPPED, ld.SILENT, ld.SHORT, ld.OK]
    peak = model.peak_normalize_int16(x.unsqueeze(1), valid=valid)
    assert torch.equal(pcm[:3], peak[:3]) and not torch.equal(pcm[3], peak[3])
    y = model.loudness_normalize(x, TARGET, valid=valid, sample_rate=rate, out="float").cpu().numpy()
    assert np.array_equal(y[0], rows[0] / np.abs(rows[0]).max()) and np.array_equal(y[1], rows[1])
    assert np.array_equal(y[2, :8819], rows[2][:8819]) and not y[2, 8819:].any()
    assert rec["gain"][0] == np.float32(1) / np.abs(rows[0]).max() and rec["gain"][1] == 1.0 and rec["gain"][2] == 1.0


@pytest.mark.gpu
def test_ragged_batches_are_batch_invariant_and_deterministic(model):
    rate, L = 22050, 3 * TILE + 4321
    kinds = ("noise", "gated", "dclf", "noise", "gated")
    valid = [L, TILE + 1, 2 * TILE + 2212, 8820, 8000]
    rng = np.random.default_rng(77)
    host = rng.standard_normal((5, L)).astype(np.float32)            # garbage behind every utterance
    for b, (k, v) in enumerate(zip(kinds, valid)):
        host[b, :v] = signal_of(k, rate, v)
    x = torch.from_numpy(host).cuda()
    rec = model.loudness(x, valid=valid, sample_rate=rate)
    pcm, rec16 = model.loudness_normalize(x, TARGET, valid=valid, sample_rate=rate, out="int16", return_record=True)
    y, rec32 = model.loudness_normalize(x, TARGET, valid=valid, sample_rate=rate, out="float", return_record=True)
    assert int(rec["status"][4]) == ld.SHORT and int(rec16["status"][2]) == ld.CLIPPED
    for b, v in enumerate(valid):
        own = x[b, :v].clone()
        r1 = model.loudness(own, sample_rate=rate)
        p1, r16 = model.loudness_normalize(own, TARGET, sample_rate=rate, out="int16", return_record=True)
        y1, r32 = model.loudness_normalize(own, TARGET, sample_rate=rate, out="float", return_record=True)
        for batch, alone in ((rec, r1), (rec16, r16), (rec32, r32)):
            for key in batch:
                assert batch[key][b].tobytes() == alone[key][0].tobytes(), (b, key, batch[key][b], alone[key][0])
        assert torch.equal(pcm[b, :v], p1[0]) and torch.equal(y[b, :v], y1), b
        assert not pcm[b, v:].any() and not y[b, v:].any(), b
    again16 = model.loudness_normalize(x, TARGET, valid=valid, sample_rate=rate, out="int16")
    again = model.loudness(x, valid=valid, sample_rate=rate)
    assert torch.equal(again16, pcm) and all(again[k].tobytes() == rec[k].tobytes() for k in rec)


@pytest.mark.gpu
def test_the_calls_capture_and_a_growing_scratch_is_refused_inside_a_capture():
    """Coefficients and powers are kernel arguments, so nothing is uploaded: the call can be recorded in a graph once its scratch buffer
    exists.  A call that would have to grow the buffer inside a capture is refused with FD_ERR_STATE."""
    import gpu_common
    m = gpu_common.make_model()                            # a handle of its own: no loudness scratch yet
    rate, n = 22050, 2 * TILE + 2212
    a = torch.from_numpy(signal_of("noise", rate, n).copy()).cuda().reshape(1, n)
    b = torch.from_numpy(signal_of("gated", rate, n).copy()).cuda().reshape(1, n)
    want_a = m.loudness_normalize(a, TARGET, sample_rate=rate, out="int16")      # (also grows the scratch buffer)
    want_b = m.loudness_normalize(b, TARGET, sample_rate=rate, out="int16")
    x = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = m.loudness_normalize(x, TARGET, sample_rate=rate, out="int16")
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want_a)
    x.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want_b)
    big = torch.zeros(4, 8 * TILE, device="cuda")
    refused = torch.cuda.CUDAGraph()
    with pytest.raises(_capi.FastDiffHipError, match="stream capture"):
        with torch.cuda.graph(refused):
            x.mul_(1.0)                                    # (so that the abandoned capture is not empty)
            m.loudness_normalize(big, TARGET, sample_rate=rate, out="int16")
    torch.cuda.synchronize()
    assert torch.equal(m.loudness_normalize(a, TARGET, sample_rate=rate, out="int16"), want_a)      # the handle works on


@pytest.mark.gpu
def test_refusals_leave_a_message(model):
    lib, h = model._ready(torch.device("cuda"))
    x = torch.zeros(1, 9000, device="cuda")
    rec = torch.empty(32, dtype=torch.uint8, device="cuda")
    assert lib.fd_loudness_measure(h, x.data_ptr(), 1, 9000, None, 7999, rec.data_ptr(), None) == _capi.FD_ERR_INVALID
    assert b"sample rate" in lib.fd_last_error(h)
    assert lib.fd_loudness_normalize(h, x.data_ptr(), 1, 9000, None, 22050, -23.0, None, None, None, None) == _capi.FD_ERR_INVALID
    assert b"neither" in lib.fd_last_error(h)
    with pytest.raises(Exception, match="valid"):
        model.loudness(x, valid=[9001])
    with pytest.raises(ValueError):
        model.loudness_normalize(x, -23.0, out="int8")
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_synthesize_to_a_loudness_target(model):
    rng = np.random.default_rng(4)
    items = [{"item_name": f"u{i}", "mel": torch.from_numpy((rng.random((t + 1, 80)) * 7.5 - 6.0).astype(np.float32)), "len": t + 1}
             for i, t in enumerate((40, 36))]
    peak = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=11)
    out = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=11, loudness=-23.0)
    assert {k: v.shape[0] for k, v in out.items()} == {"u0": 40 * 256, "u1": 36 * 256}
    for name, pcm in out.items():
        assert pcm.dtype == np.int16
        r = ref.measure(pcm.astype(np.float32) / np.float32(32767.0), 22050)
        print(f"{name}: {r['lufs']:.4f} LUFS, status {ld.STATUS[r['status']]}, peak {np.abs(pcm).max()}")
        if not (r["status"] == ref.OK and abs(r["lufs"] - (-23.0)) <= 0.01):
            assert np.array_equal(pcm, peak[name]), (name, r)      # not OK on the device: the peak epilogue's bytes
    # the rows, one by one: the float waveform of the micro-batch through the epilogue alone
    mels, lens, names = infer.collate_test_batch(items)
    rows = infer._step_rows(model, 4, None, None)
    with torch.no_grad():
        wav = model.sample(mels.cuda(), rows, ddim=False, seed=11, lens=lens, stream_ids=[0, 1])
    for b, (name, t) in enumerate(zip(names, lens)):
        want, rec = model.loudness_normalize(wav[b, 0, : t * 256].clone(), -23.0, out="int16", return_record=True)
        assert np.array_equal(out[name], want[0].cpu().numpy()), name
        if int(rec["status"][0]) != ld.OK:
            assert np.array_equal(out[name], peak[name]), name
    resampled = infer.synthesize(model, items, n_steps=4, max_batch=2, seed=11, loudness=-23.0, out_sample_rate=16000)
    for b, (name, t) in enumerate(zip(names, lens)):      # measured as delivered: after the resampling, at that rate
        own = model.resample(wav[b, 0, : t * 256].clone(), 22050, 16000)
        assert np.array_equal(resampled[name], model.loudness_normalize(own, -23.0, sample_rate=16000, out="int16")[0].cpu().numpy()), name
    long = infer.synthesize_long(model, items, n_steps=4, seed=11, loudness=-23.0)
    assert all(np.array_equal(long[k], out[k]) for k in out)


def _speechlike(rng, n):
    t = np.arange(n)
    x = 0.4 * np.sin(2 * np.pi * t / 97.0) + 0.2 * np.sin(2 * np.pi * t / 13.7) + 0.05 * rng.standard_normal(n)
    return np.round(x * 20000).astype(np.int16)


@pytest.mark.gpu
def test_load_wav_inputs_and_the_corpus_apply_loud_norm(model, tmp_path):
    rng = np.random.default_rng(21)
    pcm = _speechlike(rng, 12000)
    good = tmp_path / "good"
    good.mkdir()
    wavfile.write(good / "a.wav", 22050, pcm)
    items = infer.load_wav_inputs(model, str(good), loud_norm=True)
    want_wav, r = ref.normalize(infer.pcm_to_float(pcm), 22050, -22.0, "float")
    assert r["status"] == ref.OK
    want = model.mel_spectrogram(torch.from_numpy(want_wav).cuda())[0].transpose(0, 1).contiguous().cpu()
    d = float((items[0]["mel"] - want).abs().max())
    print(f"loud_norm mel: max |diff| {d:.2e}")
    assert items[0]["mel"].shape == want.shape and d <= 2e-4
    plain = infer.load_wav_inputs(model, str(good))
    assert float((plain[0]["mel"] - want).abs().max()) > 1e-2                 # the branch does something
    corpus = TrainCorpus.from_wav_dir(model, str(good), max_samples=2560, loud_norm=True)
    assert ulp_diff(corpus.wav[:12000].cpu().numpy(), want_wav).max() <= 2.0
    short = tmp_path / "short"
    short.mkdir()
    wavfile.write(short / "tiny.wav", 22050, pcm[:4000])
    with pytest.raises(ValueError, match="tiny.wav"):
        infer.load_wav_inputs(model, str(short), loud_norm=True)
    with pytest.raises(ValueError, match="tiny.wav"):
        TrainCorpus.from_wav_dir(model, str(short), max_samples=2560, loud_norm=True)
    silent = tmp_path / "silent"
    silent.mkdir()
    wavfile.write(silent / "z.wav", 22050, np.zeros(12000, np.int16))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        z = infer.load_wav_inputs(model, str(silent), loud_norm=True)
    assert any("z.wav" in str(w.message) for w in caught)
    assert torch.equal(z[0]["mel"], infer.load_wav_inputs(model, str(silent))[0]["mel"])
