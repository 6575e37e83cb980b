"""STOI and ESTOI on the device: how intelligible a vocoded waveform is against its recording.

The FastDiff paper's objective table reports STOI next to MOS and PESQ; the reference has no code for it (people run pystoi over the
*_gt.wav / *_pred.wav pairs that test_step writes, FastDiff.py:113-117).  Here it is one call (fd_stoi_measure,
include/fastdiff_hip_ext.h, which defines the measurement: resample to 10 kHz, drop silent frames, 512-point STFT, 15 one-third octave
bands, 384 ms segments, normalise, clip, correlate -- pystoi's conventions as recalled, with two stated deviations: the library's own
resampler, and no random noise in ESTOI's normalisation).

    bands()                      (lo, hi): the 15 bands as bin ranges [lo, hi) of the 512-point transform, from the library
    frames(n)                    the number of analysis frames of n samples at 10 kHz
    measure(clean, degraded, valid=None, sample_rate=22050)                   -> record
    STATUS                       names of the record's status values

A record is a dict of numpy arrays over the batch: stoi, estoi (float64; NaN unless OK), frames, kept, segments, status (int32).
SHORT: fewer than 31 frames survive the silence removal, so there is not one segment (pystoi returns 1e-5 with a warning); SILENT: the
clean signal is all zeros; OK otherwise.
"""
import numpy as np
import torch

from . import _capi, _wave

SCAN_TILE, SEG_TILE = _capi.FD_STOI_SCAN_TILE, _capi.FD_STOI_SEG_TILE
OK, SHORT, SILENT = _capi.FD_STOI_OK, _capi.FD_STOI_SHORT, _capi.FD_STOI_SILENT
STATUS = {OK: "OK", SHORT: "SHORT", SILENT: "SILENT"}
RECORD = _capi.record("fd_stoi")


def bands():
    """The band table as the library computes it from its rule (fd_stoi_bands): two int arrays [15]."""
    lib = _capi.load()
    lo, hi = np.zeros(15, np.int32), np.zeros(15, np.int32)
    if lib.fd_stoi_bands(lo.ctypes.data, hi.ctypes.data) != _capi.FD_OK:
        raise RuntimeError("stoi: fd_stoi_bands failed")
    return lo, hi


def frames(n):
    """Analysis frames of n samples at 10 kHz (fd_stoi_frames): len(range(0, n - 256, 128))."""
    lib = _capi.load()
    r = lib.fd_stoi_frames(int(n))
    if r < 0:
        raise ValueError(f"stoi: frames({n})")
    return int(r)


def _prepare(clean, degraded, valid):
    clean, B, L = _wave.rows(clean, "stoi", "clean")
    degraded, Bd, Ld = _wave.rows(degraded, "stoi", "degraded")
    if (Bd, Ld) != (B, L) or degraded.device != clean.device:
        raise ValueError(f"stoi: clean {list(clean.shape)} and degraded {list(degraded.shape)} must be the same batch of waveforms on one device")
    return clean, degraded, B, L, _wave.counts(valid, B, "stoi")


def _record(rec):
    return _wave.records(rec, RECORD, RECORD.names)


def _enqueue(lib, handle, stream, clean, degraded, valid, sample_rate, rec=None):
    """fd_stoi_measure on the stream -> the device records [B, 32] uint8 (`rec` to write into); nothing synchronises."""
    clean, degraded, B, L, varr = _prepare(clean, degraded, valid)
    if rec is None:
        rec = torch.empty((B, RECORD.itemsize), device=clean.device, dtype=torch.uint8)
    assert rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == B * RECORD.itemsize
    rc = lib.fd_stoi_measure(handle, clean.data_ptr(), degraded.data_ptr(), B, L, varr, int(sample_rate), rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_stoi_measure")
    return rec


def _measure(lib, handle, stream, clean, degraded, valid, sample_rate):
    return _record(_enqueue(lib, handle, stream, clean, degraded, valid, sample_rate))


def measure(clean, degraded, valid=None, sample_rate=22050):
    """clean, degraded: device tensors [n] / [B, n] / [B, 1, n] of one shape -> record of the B pairs (one synchronisation).  valid: [B]
    sample counts of a padded batch; what lies behind them is not read.  Runs on the current stream, on the per-device handle of the
    operators (lvc_op); FastDiff.stoi uses the module's own."""
    return _measure(*_wave.default_handle(clean), clean, degraded, valid, sample_rate)
