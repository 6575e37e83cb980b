"""F0 tracking on the device (YIN) and the pitch scores of a vocoded waveform against its recording.

The reference's data pipeline extracts one F0 per mel frame with Praat or WORLD (data_gen/tts/data_gen_utils.py: get_pitch, 80-750 Hz,
one value per hop).  Here the tracker is YIN (de Cheveigne and Kawahara 2002) on the same frame grid (fd_pitch_track,
include/fastdiff_hip_ext.h, which defines the measurement: the direct difference function over win samples, its cumulative mean
normalisation, the first lag below the threshold, the descent to the local minimum, a parabola), so the values differ from the
reference's binarised F0.  On the tracks of a recording and its vocoded copy, fd_pitch_compare gives what vocoder papers report next to
STOI: F0 RMSE in cents and the gross pitch error over the frames voiced in both, and the voicing decision error over all frames.

    default_config()             {"rate", "hop", "win", "f0_min", "f0_max", "threshold"} as the library fills them
    lags(cfg)                    (tau_min, tau_max); ValueError for a configuration the library refuses
    frames(n, hop)               n // hop: the F0 values of n samples
    track(wav, valid=None, **cfg)                         -> (f0, aper): device tensors [B, F]
    compare(f0_ref, f0_deg, frames=None)                  -> record
    measure(clean, degraded, valid=None, **cfg)           -> record
    STATUS                       names of the record's status values

A record is a dict of numpy arrays over the batch: rmse_cents, gpe, vde (float64), frames, both_voiced, ref_voiced, deg_voiced, status
(int32).  SHORT: not one frame, all three NaN; UNVOICED: no frame is voiced in both tracks, vde is valid and the other two NaN; OK
otherwise.
"""
import ctypes as ct

import torch

from . import _capi, _wave

MAX_LAGS, FRAME_TILE, LAG_CHUNK, STAGE_FLOATS = _capi.FD_PITCH_MAX_LAGS, _capi.FD_PITCH_FRAME_TILE, _capi.FD_PITCH_LAG_CHUNK, _capi.FD_PITCH_STAGE_FLOATS
OK, SHORT, UNVOICED = _capi.FD_PITCH_OK, _capi.FD_PITCH_SHORT, _capi.FD_PITCH_UNVOICED
STATUS = {OK: "OK", SHORT: "SHORT", UNVOICED: "UNVOICED"}
RECORD = _capi.record("fd_pitch")
FIELDS = tuple(k for k in RECORD.names if k != "reserved")
FdPitchConfig = _capi.struct("fd_pitch_config")
KEYS = ("rate", "hop", "win", "f0_min", "f0_max", "threshold")


def _config(cfg):
    """The library's defaults with `cfg` (a dict of some of KEYS) on top, as the C structure."""
    c = FdPitchConfig()
    if _capi.load().fd_pitch_default_config(ct.byref(c)) != _capi.FD_OK:
        raise RuntimeError("pitch: fd_pitch_default_config failed")
    for k, v in (cfg or {}).items():
        if k not in KEYS:
            raise TypeError(f"pitch: unknown configuration key {k!r} (one of {', '.join(KEYS)})")
        setattr(c, k, float(v) if k in ("f0_min", "f0_max", "threshold") else int(v))
    return c


def default_config():
    c = _config(None)
    return {k: getattr(c, k) for k in KEYS}


def lags(cfg=None):
    """(tau_min, tau_max) = (floor(rate / f0_max), ceil(rate / f0_min)) of a configuration (fd_pitch_lags)."""
    c = _config(cfg)
    lo, hi = ct.c_int(0), ct.c_int(0)
    if _capi.load().fd_pitch_lags(ct.byref(c), ct.byref(lo), ct.byref(hi)) != _capi.FD_OK:
        raise ValueError(f"pitch: the configuration {({k: getattr(c, k) for k in KEYS})} is refused")
    return lo.value, hi.value


def frames(n, hop=256):
    """F0 values of n samples (fd_pitch_frames): n // hop, the mel frame count for n = T * hop."""
    r = _capi.load().fd_pitch_frames(int(n), int(hop))
    if r < 0:
        raise ValueError(f"pitch: frames({n}, {hop})")
    return int(r)


def _track(lib, handle, stream, wav, valid, cfg):
    """fd_pitch_track on the stream -> (f0, aper) device [B, F]; nothing synchronises."""
    c = cfg if isinstance(cfg, FdPitchConfig) else _config(cfg)
    wav, B, L = _wave.rows(wav, "pitch")
    varr = _wave.counts(valid, B, "pitch")
    F = L // max(int(c.hop), 1)
    out = torch.zeros((2, B, max(F, 1)), device=wav.device, dtype=torch.float32)
    rc = lib.fd_pitch_track(handle, wav.data_ptr(), B, L, varr, ct.byref(c), out[0].data_ptr(), out[1].data_ptr(), max(F, 1), stream)
    _capi.check(lib, handle, rc, "fd_pitch_track")
    return out[0, :, :F], out[1, :, :F]


def _record(rec):
    return _wave.records(rec, RECORD, FIELDS)


def _compare(lib, handle, stream, f0_ref, f0_deg, nframes=None, rec=None):
    """fd_pitch_compare on the stream -> the device records [B, 48] uint8 (`rec` to write into); nothing synchronises.  Two tracks
    without a frame give SHORT records without a launch argument of size zero: the row pitch is at least 1."""
    if f0_ref.dim() != 2 or f0_ref.shape != f0_deg.shape or f0_ref.device != f0_deg.device:
        raise ValueError(f"pitch: two tracks [B, F] of one shape on one device are expected, got {list(f0_ref.shape)} and {list(f0_deg.shape)}")
    B, F = f0_ref.shape
    if nframes is None:
        nframes = [F] * B
    if F == 0:      # (the views of _track's buffer: one column stands behind them, but a caller's empty tensor has none)
        f0_ref = f0_deg = torch.zeros((B, 1), device=f0_ref.device, dtype=torch.float32)
    a, B, pitch = _wave.rows(f0_ref, "pitch", "track")
    g = _wave.rows(f0_deg, "pitch", "track")[0]
    farr = _wave.counts(nframes, B, "pitch")
    if rec is None:
        rec = torch.empty((B, RECORD.itemsize), device=a.device, dtype=torch.uint8)
    assert rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == B * RECORD.itemsize
    rc = lib.fd_pitch_compare(handle, a.data_ptr(), g.data_ptr(), B, pitch, farr, rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_pitch_compare")
    return rec


def _enqueue(lib, handle, stream, clean, degraded, valid, cfg, rec=None):
    """Both tracks and their comparison on the stream -> the device records [B, 48] uint8; nothing synchronises."""
    c = cfg if isinstance(cfg, FdPitchConfig) else _config(cfg)
    if not isinstance(clean, torch.Tensor) or not isinstance(degraded, torch.Tensor) or clean.numel() != degraded.numel() or clean.device != degraded.device:
        raise ValueError("pitch: clean and degraded must be the same batch of waveforms on one device")
    f_ref = _track(lib, handle, stream, clean, valid, c)[0]
    f_deg = _track(lib, handle, stream, degraded, valid, c)[0]
    if f_ref.shape != f_deg.shape:
        raise ValueError(f"pitch: clean {list(clean.shape)} and degraded {list(degraded.shape)} must be the same batch of waveforms")
    nframes = None if valid is None else [int(v) // int(c.hop) for v in valid]
    return _compare(lib, handle, stream, f_ref, f_deg, nframes, rec)


def _measure(lib, handle, stream, clean, degraded, valid, cfg):
    return _record(_enqueue(lib, handle, stream, clean, degraded, valid, cfg))


def track(wav, valid=None, **cfg):
    """wav: device tensor [n] / [B, n] / [B, 1, n] -> (f0, aper), device float32 [B, n // hop]: f0 in Hz, 0 where unvoiced; aper = d' at
    the chosen lag (its minimum over the lag range where unvoiced).  valid: [B] sample counts of a padded batch; what lies behind them
    is not read, and the frames behind valid[b] // hop are (0, 1).  cfg: rate, hop, win, f0_min, f0_max, threshold.  Runs on the current
    stream, on the per-device handle of the operators (lvc_op); FastDiff.pitch_track uses the module's own.  Does not synchronise."""
    lib, h, stream = _wave.default_handle(wav)
    return _track(lib, h, stream, wav, valid, cfg)


def compare(f0_ref, f0_deg, frames=None):
    """Two device tracks [B, F] (or [F]) -> record (one synchronisation).  frames: [B] frame counts of a padded batch."""
    if f0_ref.dim() == 1:
        f0_ref, f0_deg = f0_ref.unsqueeze(0), f0_deg.unsqueeze(0)
    lib, h, stream = _wave.default_handle(f0_ref)
    return _record(_compare(lib, h, stream, f0_ref, f0_deg, frames))


def measure(clean, degraded, valid=None, **cfg):
    """clean, degraded: device tensors [n] / [B, n] / [B, 1, n] of one shape -> record of the B pairs (one synchronisation)."""
    lib, h, stream = _wave.default_handle(clean)
    return _measure(lib, h, stream, clean, degraded, valid, cfg)
