"""Cutting long silences on the device: the `trim_long_sil` switch of the reference's process_utterance.

The reference (data_gen/tts/data_gen_utils.py:27-90, trim_long_silences) loud-normalises a recording to -20 LUFS, flags 30 ms windows as
speech or not with WebRTC's detector at 16 kHz, smooths the flags with an 8-window moving average, dilates them so that a pause of up to
12 windows survives, and removes every sample that is not under the mask.  Here that is one call (fd_trim_silences,
include/fastdiff_hip_ext.h, which defines the method).  The smoothing and the dilation are the reference's, in integers.  The detector is
NOT WebRTC's sub-band GMM: it is an energy detector (a window is speech when its level lies within top_db of the loudest window and above
floor_db), on the native rate's window grid (661 samples at 22050 Hz) instead of a 16 kHz copy -- webrtcvad cannot be run here, so the
flags are not claimed to be close to its flags.  The output is a bit copy of input samples; nothing is scaled or filtered.

    windows(n, rate, window_ms=30)          (W, M): the window in samples and the windows of n samples, from the library
    trim(wav, valid=None, sample_rate=22050, window_ms=30, top_db=40., floor_db=-70., average_width=8, max_silence=12, mode="long",
         return_flags=False, return_record=False) -> (out [B, L], out_valid device int32 [B]) [, flags] [, record]
    levels(wav, valid=None, sample_rate=22050, window_ms=30) -> device float64 [B, Mmax]: each window's level in dB re full scale
    mask(speech, average_width=8, max_silence=12, mode="long") -> flags (numpy uint8): the library's host statement of steps 4-5
    STATUS                                   names of the record's status values

out holds each utterance's kept samples in order and 0 behind them; out_valid their count (on the device: nothing synchronises without
return_record).  flags: device uint8 [B, Mmax], bit 0 speech, bit 1 smoothed, bit 2 kept, 0 behind an utterance's own windows.  A record
is a dict of numpy arrays over the batch: n_out, windows, speech, kept_windows, nonfinite, status (int32), peak_db, threshold_db
(float64).  SILENT: no window is kept, n_out = 0 (the reference would return an empty array); EMPTY: valid[b] = 0.
"""
import ctypes as ct

import numpy as np
import torch

from . import _capi, _wave

CHUNK = _capi.FD_TRIM_CHUNK
OK, SILENT, EMPTY = _capi.FD_TRIM_OK, _capi.FD_TRIM_SILENT, _capi.FD_TRIM_EMPTY
STATUS = {OK: "OK", SILENT: "SILENT", EMPTY: "EMPTY"}
MODES = {"long": _capi.FD_TRIM_LONG, "edges": _capi.FD_TRIM_EDGES}
RECORD = _capi.record("fd_trim")
SPEECH, SMOOTH, KEEP = 1, 2, 4


def windows(n, rate, window_ms=30):
    """(W, M) of n samples at `rate` (fd_trim_windows)."""
    lib = _capi.load()
    W, M = ct.c_int64(), ct.c_int64()
    if lib.fd_trim_windows(int(n), int(rate), int(window_ms), ct.byref(W), ct.byref(M)) != _capi.FD_OK:
        raise ValueError(f"trim: windows({n}, {rate}, {window_ms}): n >= 0, a rate of 8000 .. 192000 and window_ms 10, 20 or 30 are expected")
    return int(W.value), int(M.value)


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f"trim: mode must be 'long' or 'edges', got {mode!r}")
    return MODES[mode]


def mask(speech, average_width=8, max_silence=12, mode="long"):
    """Steps 4-5 as the library states them on the host (fd_trim_mask): speech flags [M] -> flags [M] (SPEECH | SMOOTH | KEEP bits)."""
    lib = _capi.load()
    s = np.ascontiguousarray(np.asarray(speech) != 0, dtype=np.uint8)
    out = np.zeros(len(s), np.uint8)
    if lib.fd_trim_mask(s.ctypes.data, len(s), int(average_width), int(max_silence), _mode(mode), out.ctypes.data) != _capi.FD_OK:
        raise ValueError(f"trim: mask of {len(s)} windows with average_width {average_width}, max_silence {max_silence} refused")
    return out


def _record(rec):
    return _wave.records(rec, RECORD, ("n_out", "windows", "speech", "kept_windows", "nonfinite", "status", "peak_db", "threshold_db"))


def _params(sample_rate, window_ms, top_db, floor_db, average_width, max_silence, mode):
    return _capi.FdTrimParams(int(sample_rate), int(window_ms), int(average_width), int(max_silence), _mode(mode), 0, float(top_db), float(floor_db))


def _trim(lib, handle, stream, wav, valid, sample_rate, window_ms, top_db, floor_db, average_width, max_silence, mode, return_flags, return_record):
    wav, B, L = _wave.rows(wav, "trim")
    varr = _wave.counts(valid, B, "trim")
    p = _params(sample_rate, window_ms, top_db, floor_db, average_width, max_silence, mode)
    out = torch.empty((B, L), device=wav.device, dtype=torch.float32)
    out_valid = torch.empty((B,), device=wav.device, dtype=torch.int32)
    flags = rec = None
    if return_flags:
        flags = torch.empty((B, windows(L, sample_rate, window_ms)[1]), device=wav.device, dtype=torch.uint8)
    if return_record:
        rec = torch.empty((B, RECORD.itemsize), device=wav.device, dtype=torch.uint8)
    rc = lib.fd_trim_silences(handle, wav.data_ptr(), B, L, varr, ct.byref(p), out.data_ptr(), out_valid.data_ptr(),
                              flags.data_ptr() if return_flags else None, rec.data_ptr() if return_record else None, stream)
    _capi.check(lib, handle, rc, "fd_trim_silences")
    ret = (out, out_valid)
    if return_flags:
        ret += (flags,)
    if return_record:
        ret += (_record(rec),)
    return ret


def _levels(lib, handle, stream, wav, valid, sample_rate, window_ms):
    wav, B, L = _wave.rows(wav, "trim")
    varr = _wave.counts(valid, B, "trim")
    lv = torch.empty((B, windows(L, sample_rate, window_ms)[1]), device=wav.device, dtype=torch.float64)
    rc = lib.fd_trim_levels(handle, wav.data_ptr(), B, L, varr, int(sample_rate), int(window_ms), lv.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_trim_levels")
    return lv


def trim(wav, valid=None, sample_rate=22050, window_ms=30, top_db=40., floor_db=-70., average_width=8, max_silence=12, mode="long",
         return_flags=False, return_record=False):
    """wav: device tensor [n] / [B, n] / [B, 1, n] -> (out [B, n] float32, out_valid device int32 [B]), then the flags and the record
    on request.  valid: [B] sample counts of a padded batch (0 allowed: EMPTY); what lies behind them is not read.  mode "long": the
    reference's mask; "edges": everything from the first kept window to the last.  An utterance's result does not depend on the batch it
    is in.  Without return_record the call is asynchronous and can be captured into a graph.  Runs on the current stream, on the
    per-device handle of the operators (lvc_op); FastDiff.trim_silences uses the module's own."""
    return _trim(*_wave.default_handle(wav), wav, valid, sample_rate, window_ms, top_db, floor_db, average_width, max_silence, mode,
                 return_flags, return_record)


def levels(wav, valid=None, sample_rate=22050, window_ms=30):
    """The level of every window, dB re full scale: device float64 [B, Mmax]; NaN for a window that holds a sample that is not finite, 0
    behind an utterance's own windows."""
    return _levels(*_wave.default_handle(wav), wav, valid, sample_rate, window_ms)
