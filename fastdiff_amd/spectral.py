"""Multi-resolution STFT distances on the device: how close the spectrum of a vocoded waveform is to its recording's.

Vocoder papers since Parallel WaveGAN report the multi-resolution STFT error (spectral convergence plus log-magnitude distance at three
window sizes) and the log-spectral distance; the reference ships modules/parallel_wavegan without its STFT loss and utils/torch_stft.py
without a caller, so people compute them offline with torch over the *_gt.wav / *_pred.wav pairs that test_step writes.  Here it is one
call (fd_spectral_measure, include/fastdiff_hip_ext.h, which defines the measurement: torch.stft's conventions -- centred frames, reflect
padding, periodic Hann window -- magnitudes with a power floor, then sc = sqrt(sum (X - Y)^2 / sum X^2), logmag = mean |ln X - ln Y| in
nepers and lsd = mean_f sqrt(mean_k (20 log10 X - 20 log10 Y)^2) in dB per resolution).  The 2048-point resolution shows over-smoothed
harmonics, the 512-point one at hop 50 smeared transients and pre-echo from too few reverse steps.

    default_config()             {"resolutions": ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200)), "floor": 1e-7}, from the library
    frames(n, hop)               the number of frames of n samples: 1 + n // hop
    measure(clean, degraded, valid=None, resolutions=..., floor=...)          -> record
    STATUS                       names of the record's status values

resolutions: 1 .. 4 of (nfft, hop, win) in samples, whatever the rate: nfft 512, 1024 or 2048, 2 <= win <= nfft, 16 <= hop <= nfft.
A record is a dict of numpy arrays over the batch: sc, logmag, lsd [B, 4] (float64, per resolution; NaN beyond the configured ones),
mr_sc, mr_logmag, lsd_db [B] (their means over the resolutions), frames [B, 4], n_res, status (int32).  SHORT: the pair has at most
max nfft / 2 samples, where the reflection is undefined, and every value is NaN; OK otherwise (the floor keeps silence measurable).  A
copy scores exactly 0.
"""
import ctypes as ct

import torch

from . import _capi, _wave

MAX_RES, FRAME_TILE, SUM_CHUNK = _capi.FD_SPECTRAL_MAX_RES, _capi.FD_SPECTRAL_FRAME_TILE, _capi.FD_SPECTRAL_SUM_CHUNK
OK, SHORT = _capi.FD_SPECTRAL_OK, _capi.FD_SPECTRAL_SHORT
STATUS = {OK: "OK", SHORT: "SHORT"}
RECORD = _capi.record("fd_spectral")
FdSpectralConfig = _capi.struct("fd_spectral_config")
KEYS = ("resolutions", "floor")


def _config(cfg):
    """The library's defaults with `cfg` (a dict of some of KEYS) on top, as the C structure.  The values are the library's to refuse; only
    a list that does not fit the structure is refused here."""
    c = FdSpectralConfig()
    if _capi.load().fd_spectral_default_config(ct.byref(c)) != _capi.FD_OK:
        raise RuntimeError("spectral: fd_spectral_default_config failed")
    for k, v in (cfg or {}).items():
        if k not in KEYS:
            raise TypeError(f"spectral: unknown configuration key {k!r} (one of {', '.join(KEYS)})")
        if k == "floor":
            c.floor = float(v)
            continue
        res = [tuple(int(a) for a in r) for r in v]
        if any(len(r) != 3 for r in res):
            raise ValueError(f"spectral: a resolution is (nfft, hop, win), got {res}")
        c.n_res = len(res)      # (the library refuses 0 and more than MAX_RES, by name)
        for r in range(MAX_RES):
            c.nfft[r], c.hop[r], c.win[r] = res[r] if r < len(res) else (0, 0, 0)
    return c


def default_config():
    c = _config(None)
    return {"resolutions": tuple((c.nfft[r], c.hop[r], c.win[r]) for r in range(c.n_res)), "floor": c.floor}


def frames(n, hop):
    """Frames of n samples at `hop` (fd_spectral_frames): 1 + n // hop, torch.stft's count with center=True."""
    r = _capi.load().fd_spectral_frames(int(n), int(hop))
    if r < 0:
        raise ValueError(f"spectral: frames({n}, {hop})")
    return int(r)


def _prepare(clean, degraded, valid):
    clean, B, L = _wave.rows(clean, "spectral", "clean")
    degraded, Bd, Ld = _wave.rows(degraded, "spectral", "degraded")
    if (Bd, Ld) != (B, L) or degraded.device != clean.device:
        raise ValueError(f"spectral: clean {list(clean.shape)} and degraded {list(degraded.shape)} must be the same batch of waveforms on one device")
    return clean, degraded, B, L, _wave.counts(valid, B, "spectral")


def _record(rec):
    return _wave.records(rec, RECORD, RECORD.names)


def _enqueue(lib, handle, stream, clean, degraded, valid, cfg, rec=None):
    """fd_spectral_measure on the stream -> the device records [B, 144] uint8 (`rec` to write into); nothing synchronises."""
    c = cfg if isinstance(cfg, FdSpectralConfig) else _config(cfg)
    clean, degraded, B, L, varr = _prepare(clean, degraded, valid)
    if rec is None:
        rec = torch.empty((B, RECORD.itemsize), device=clean.device, dtype=torch.uint8)
    assert rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == B * RECORD.itemsize
    rc = lib.fd_spectral_measure(handle, clean.data_ptr(), degraded.data_ptr(), B, L, varr, ct.byref(c), rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_spectral_measure")
    return rec


def _measure(lib, handle, stream, clean, degraded, valid, cfg):
    return _record(_enqueue(lib, handle, stream, clean, degraded, valid, cfg))


def measure(clean, degraded, valid=None, **cfg):
    """clean, degraded: device tensors [n] / [B, n] / [B, 1, n] of one shape -> record of the B pairs (one synchronisation).  valid: [B]
    sample counts of a padded batch; what lies behind them is not read.  cfg: resolutions, floor.  Runs on the current stream, on the
    per-device handle of the operators (lvc_op); FastDiff.spectral uses the module's own."""
    return _measure(*_wave.default_handle(clean), clean, degraded, valid, cfg)
