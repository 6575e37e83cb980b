"""Cases of the guarded-memory suite (tests/guarded_suite.py): the waveform tools in front of and behind the vocoder.
"""
import numpy as np
import torch

from fastdiff_amd import _capi
from guarded_suite import as_tensors, case, model, rnd

HOST_BANK = "a host array (numpy) into which the wrapper itself reads the handle's filter bank; the library uses it on the host"
HOST_PINV = "a host array (numpy) the wrapper computes itself from the handle's filter bank; the library reads it on the host"

# =====================================================================================================================================
# Waveform tools: batches of 3 with `valid`, the shortest item first and last
# =====================================================================================================================================
def _wave(seed, B, n, scale=0.3):
    return rnd(seed, B, n, scale=scale).clamp_(-1, 1)


def _orders(lengths):
    """(tag, valid) for the shortest item first and for it last; `lengths` ascending."""
    return (("-short-first", list(lengths)), ("-short-last", list(lengths[::-1])))


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
        for tag, valid in _orders((lo // 2, lo, hi)):
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
    for tag, valid in _orders((8820, _capi.FD_LOUDNESS_TILE, n)):          # one gating block; the tile; one sample into the second tile
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
    for tag, valid in _orders((256, 4097, 4225)):          # STEADY_LENGTHS: the shortest, and two around a border
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
    for tag, valid in _orders([f * hop for f in frames]):
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
    for tag, valid in _orders((1024, 1025, 2049)):          # LENGTHS: the shortest, and its neighbours of two borders
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
        for tag, lens in _orders((2, max(2, T - 1), T)):
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
    for tag, lens in _orders((1, _capi.FD_NNLS_FRAME_TILE, _capi.FD_NNLS_FRAME_TILE + 1)):
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
    for tag, valid in _orders((1, 513, L)):
        out["ragged" + tag] = m.peak_normalize_int16(g.tensor(_padded(rnd(2, 3, L), valid).view(3, 1, L)), valid=valid)
    lib, h = m._ready(wav.device)                      # the entry point without `valid`, which the wrapper reaches through its ragged twin
    pcm = torch.empty((3, L), device=wav.device, dtype=torch.int16)
    _capi.check(lib, h, lib.fd_peak_normalize_int16(h, wav.data_ptr(), 3, L, pcm.data_ptr(), lvc_op._stream(wav.device)), "fd_peak_normalize_int16")
    out["c-plain"] = pcm
    return out
