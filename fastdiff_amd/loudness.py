"""BS.1770 loudness on the device: measure a waveform's integrated loudness and normalise it to a target.

The reference normalises a recording to -22 LUFS in front of the mel (`process_utterance(loud_norm=True)`,
data_gen/tts/data_gen_utils.py:115-120: pyloudnorm.Meter(rate) with its defaults, one channel; trim_long_silences(norm=True), :42-47,
to -20); behind the vocoder its only level control is wav / abs(wav).max() (FastDiff.py:110).  Here both are one call
(fd_loudness_measure / fd_loudness_normalize, include/fastdiff_hip_ext.h, which defines the measurement): K-weighting by two RBJ
biquads (pyloudnorm's, not the ITU table's: a full-scale 997 Hz sine reads -3.07 LUFS at 22050 Hz, not -3.01), 400 ms blocks every
100 ms, the absolute gate at -70 LUFS and the relative one 10 LU below the gated mean.

    design(rate)                 the ten coefficients, from the library (shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2)
    blocks(n, rate)              the number of gating blocks of n samples, 0 if too short to measure
    measure(wav, valid=None, sample_rate=22050)                               -> record
    normalize(wav, target, valid=None, sample_rate=22050, out="float"|"int16", return_record=False)
    STATUS                       names of the record's status values

A record is a dict of numpy arrays over the batch: lufs (float64; -inf for SHORT and SILENT), gain, peak (float32), blocks, gated,
status (int32).  SHORT: shorter than one block (pyloudnorm raises); SILENT: no block passes the gates; CLIPPED: peak gain > 1, so the
utterance was divided by its peak instead (data_gen_utils.py:119-120); OK otherwise.
"""
import numpy as np
import torch

from . import _capi, _wave

TILE = _capi.FD_LOUDNESS_TILE
OK, SHORT, SILENT, CLIPPED = _capi.FD_LOUDNESS_OK, _capi.FD_LOUDNESS_SHORT, _capi.FD_LOUDNESS_SILENT, _capi.FD_LOUDNESS_CLIPPED
STATUS = {OK: "OK", SHORT: "SHORT", SILENT: "SILENT", CLIPPED: "CLIPPED"}
RECORD = _capi.record("fd_loudness")


def design(rate):
    """The K-weighting coefficients at `rate` as the library computes them (fd_loudness_design), float64 [10]."""
    lib = _capi.load()
    c = np.zeros(10, np.float64)
    if lib.fd_loudness_design(int(rate), c.ctypes.data) != _capi.FD_OK:
        raise ValueError(f"loudness: sample rate {rate} outside 8000 .. 192000")
    return c


def blocks(n, rate):
    """Gating blocks of n samples at `rate` (fd_loudness_blocks); 0: shorter than one block."""
    lib = _capi.load()
    r = lib.fd_loudness_blocks(int(n), int(rate))
    if r < 0:
        raise ValueError(f"loudness: blocks({n}, {rate})")
    return int(r)


def _prepare(wav, valid, who):
    wav, B, L = _wave.rows(wav, who)
    return wav, B, L, _wave.counts(valid, B, who)


def _record(rec):
    return _wave.records(rec, RECORD, ("lufs", "gain", "peak", "blocks", "gated", "status"))


def _measure(lib, handle, stream, wav, valid, sample_rate):
    wav, B, L, varr = _prepare(wav, valid, "loudness")
    rec = torch.empty((B, RECORD.itemsize), device=wav.device, dtype=torch.uint8)
    rc = lib.fd_loudness_measure(handle, wav.data_ptr(), B, L, varr, int(sample_rate), rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_loudness_measure")
    return _record(rec)


def _normalize(lib, handle, stream, wav, target, valid, sample_rate, out, return_record):
    if out not in ("float", "int16"):
        raise ValueError(f"loudness_normalize: out must be 'float' or 'int16', got {out!r}")
    shape = wav.shape if isinstance(wav, torch.Tensor) else None
    wav, B, L, varr = _prepare(wav, valid, "loudness_normalize")
    y = torch.empty((B, L), device=wav.device, dtype=torch.float32 if out == "float" else torch.int16)
    rec = torch.empty((B, RECORD.itemsize), device=wav.device, dtype=torch.uint8) if return_record else None
    rc = lib.fd_loudness_normalize(handle, wav.data_ptr(), B, L, varr, int(sample_rate), float(target), y.data_ptr() if out == "float" else None,
                                   y.data_ptr() if out == "int16" else None, rec.data_ptr() if return_record else None, stream)
    _capi.check(lib, handle, rc, "fd_loudness_normalize")
    if out == "float" and len(shape) != 2:
        y = y.reshape(shape)
    return (y, _record(rec)) if return_record else y


def measure(wav, valid=None, sample_rate=22050):
    """wav: device tensor [n] / [B, n] / [B, 1, n] -> record of its B utterances (one synchronisation).  valid: [B] sample counts of a
    padded batch; what lies behind them is not read.  Runs on the current stream, on the per-device handle of the operators (lvc_op);
    FastDiff.loudness uses the module's own."""
    return _measure(*_wave.default_handle(wav), wav, valid, sample_rate)


def normalize(wav, target, valid=None, sample_rate=22050, out="float", return_record=False):
    """wav scaled to `target` LUFS: out="float" float32 in the shape of wav (SHORT and SILENT utterances unchanged, CLIPPED ones divided
    by their peak), out="int16" PCM [B, n] = (int16)(wav gain 32767) (SHORT, SILENT and CLIPPED ones exactly as peak_normalize_int16
    converts them); 0 behind valid[b].  An utterance's result does not depend on the batch it is in.  return_record: (output, record),
    which synchronises; without it the call is asynchronous."""
    return _normalize(*_wave.default_handle(wav), wav, target, valid, sample_rate, out, return_record)
