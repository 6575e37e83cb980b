"""Mel-cepstral distortion with time alignment on the device: the MCD column of the vocoder tables.

MCD is the number most TTS and vocoder papers quote first, and the one score here that does not compare frame i with frame i: the two
cepstral sequences are aligned by dynamic time warping first, so a waveform that is shifted or stretched by a few frames (a streaming
window, another vocoder, anything that came through an acoustic model) is not scored as wrong everywhere.  The reference has no MCD; its
alignment (utils/pitch_distance.py: time_warp, align_from_distances) is a numba double loop on the CPU.  Here it is three calls
(include/fastdiff_hip_ext.h, which defines them: fd_cepstra, fd_dtw, fd_mcd_measure):

    default_config()             {"n_coef": 13}, from the library
    frames(n)                    the number of frames of n samples: 1 + n // 256
    cepstra(wav, valid=None, n_coef=13, variant="pwg")                  -> [B, T, n_coef] device float32
    dtw(a, b, frames_a=None, frames_b=None, align=False)                -> record (, alignment [B, Ta] int32 on the device)
    measure(clean, degraded, valid=None, valid_degraded=None, n_coef=13, variant="pwg")       -> record
    STATUS                       names of the record's status values

cepstra: the log-mel of the front-end `variant` (fd_mel_spectrogram's frames, filter bank and log) as natural logarithms through the
orthonormal DCT-II over the 80 bands, coefficients 1 .. n_coef (c_0, the gain, is dropped).  This is the cepstrum of the mel filter bank,
NOT the SPTK / WORLD mcep: the values are comparable among runs of this tool.  Row t of item b behind its own 1 + valid[b] // 256 frames
is zero.
dtw: a [B, Ta, D] and b [B, Tb, D] device float32 (D <= 40; the last dimension contiguous, any row stride), Euclidean local cost in
float32, the textbook recurrence in float64, ties to the first of (diagonal, i - 1, j - 1).  The record: cost, path_len, n_diag, frames_a,
frames_b, status.  align=True also returns, for each i, the smallest j with (i, j) on the path (-1 behind frames_a[b]).
measure: cepstra of both, the alignment, and with K = 10 sqrt(2) / ln 10 the record: mcd_dtw = K cost / path_len, mcd_linear = K times the
mean distance of the frames i < min(Tc, Td) without alignment, cost, path_len, n_diag, frames_clean, frames_degraded, status.  clean and
degraded may differ in length.  A copy scores exactly 0.  SHORT: tacotron front-end and at most 512 samples; NONFINITE: a value that is
not finite; the values are then NaN.
"""
import ctypes as ct

import numpy as np
import torch

from . import _capi, _wave

MAX_COEF, MAX_FRAMES, ROWS, COLS, MAX_ALIGN_CELLS = (_capi.FD_MCD_MAX_COEF, _capi.FD_MCD_MAX_FRAMES, _capi.FD_DTW_ROWS, _capi.FD_DTW_COLS,
                                                      _capi.FD_DTW_MAX_ALIGN_CELLS)
OK, SHORT, NONFINITE = _capi.FD_MCD_OK, _capi.FD_MCD_SHORT, _capi.FD_MCD_NONFINITE
STATUS = {OK: "OK", SHORT: "SHORT", NONFINITE: "NONFINITE"}
RECORD, DTW_RECORD = _capi.record("fd_mcd"), _capi.record("fd_dtw_rec")
FIELDS = tuple(k for k in RECORD.names if k != "reserved")
DTW_FIELDS = tuple(k for k in DTW_RECORD.names if k != "reserved")
K_DB = 10.0 * np.sqrt(2.0) / np.log(10.0)
FdMcdConfig = _capi.struct("fd_mcd_config")
KEYS = ("n_coef", "variant")
VARIANTS = ("pwg", "tacotron")


def _config(cfg):
    """The library's defaults with `cfg` (a dict of some of KEYS) on top: (the C structure, the front-end's name).  The values are the
    library's to refuse."""
    c = FdMcdConfig()
    if _capi.load().fd_mcd_default_config(ct.byref(c)) != _capi.FD_OK:
        raise RuntimeError("mcd: fd_mcd_default_config failed")
    variant = "pwg"
    for k, v in (cfg or {}).items():
        if k not in KEYS:
            raise TypeError(f"mcd: unknown configuration key {k!r} (one of {', '.join(KEYS)})")
        if k == "variant":
            if v not in VARIANTS:
                raise ValueError(f"mcd: variant must be 'pwg' or 'tacotron', got {v!r}")
            variant = v
        else:
            c.n_coef = int(v)
    return c, variant


def default_config():
    return {"n_coef": _config(None)[0].n_coef}


def frames(n):
    """Frames of n samples (fd_mcd_frames): 1 + n // 256, the mel front-end's count."""
    r = _capi.load().fd_mcd_frames(int(n))
    if r < 0:
        raise ValueError(f"mcd: frames({n})")
    return int(r)


def _front_end(lib, handle, variant):
    _capi.check(lib, handle, lib.fd_set_option(handle, b"mel", variant.encode()), "fd_set_option")


def _cepstra(lib, handle, stream, wav, valid, n_coef, variant):
    wav, B, L = _wave.rows(wav, "mcd", "wav")
    T = frames(L)
    out = torch.empty((B, T, max(int(n_coef), 1)), device=wav.device, dtype=torch.float32)
    _front_end(lib, handle, variant)
    rc = lib.fd_cepstra(handle, wav.data_ptr(), B, L, _wave.counts(valid, B, "mcd"), int(n_coef), out.data_ptr(), T, stream)
    _capi.check(lib, handle, rc, "fd_cepstra")
    return out


def _rows3(t, what):
    """A device tensor [T, D] / [B, T, D] of float32 with a contiguous last dimension and uniform strides -> (it, B, T, D, ld)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("mcd: a tensor on the HIP device is expected (there is no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"mcd: {what} of shape {list(t.shape)}: [T, D] or [B, T, D] is expected")
    B, T, D = t.shape
    ld = t.stride(1) if T > 1 else max(t.stride(1), D)
    if t.stride(2) != 1 or ld < D or (B > 1 and t.stride(0) != T * ld):
        t = t.contiguous()
        ld = D
    return t, B, T, D, ld


def _dtw(lib, handle, stream, a, b, frames_a, frames_b, align):
    a, B, Ta, D, ld = _rows3(a, "a")
    b, Bb, Tb, Db, ldb = _rows3(b, "b")
    if (Bb, Db) != (B, D) or b.device != a.device:
        raise ValueError(f"mcd: a {list(a.shape)} and b {list(b.shape)} must be the same batch of D-float rows on one device")
    if ldb != ld:      # one ld for both: the wider one is repacked
        a, b, ld = a.contiguous(), b.contiguous(), D
    rec = torch.empty((B, DTW_RECORD.itemsize), device=a.device, dtype=torch.uint8)
    al = torch.empty((B, Ta), device=a.device, dtype=torch.int32) if align else None
    rc = lib.fd_dtw(handle, a.data_ptr(), b.data_ptr(), B, D, ld, Ta, Tb, _wave.counts(frames_a, B, "mcd"), _wave.counts(frames_b, B, "mcd"),
                    rec.data_ptr(), al.data_ptr() if align else None, Ta if align else 0, stream)
    _capi.check(lib, handle, rc, "fd_dtw")
    out = _wave.records(rec, DTW_RECORD, DTW_FIELDS)
    return (out, al) if align else out


def _prepare(clean, degraded, valid, valid_degraded):
    clean, B, Lc = _wave.rows(clean, "mcd", "clean")
    degraded, Bd, Ld = _wave.rows(degraded, "mcd", "degraded")
    if Bd != B or degraded.device != clean.device:
        raise ValueError(f"mcd: clean {list(clean.shape)} and degraded {list(degraded.shape)} must be the same batch of waveforms on one device")
    if valid_degraded is None:
        valid_degraded = valid      # one set of counts for both
    return clean, degraded, B, Lc, Ld, _wave.counts(valid, B, "mcd"), _wave.counts(valid_degraded, B, "mcd")


def _record(rec):
    return _wave.records(rec, RECORD, FIELDS)


def _enqueue(lib, handle, stream, clean, degraded, valid, cfg, rec=None, valid_degraded=None):
    """fd_mcd_measure on the stream -> the device records [B, 48] uint8 (`rec` to write into); nothing synchronises."""
    c, variant = cfg if isinstance(cfg, tuple) else _config(cfg)
    clean, degraded, B, Lc, Ld, va, vb = _prepare(clean, degraded, valid, valid_degraded)
    if rec is None:
        rec = torch.empty((B, RECORD.itemsize), device=clean.device, dtype=torch.uint8)
    assert rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == B * RECORD.itemsize
    _front_end(lib, handle, variant)
    rc = lib.fd_mcd_measure(handle, clean.data_ptr(), Lc, degraded.data_ptr(), Ld, B, va, vb, ct.byref(c), rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_mcd_measure")
    return rec


def _measure(lib, handle, stream, clean, degraded, valid, cfg, valid_degraded=None):
    return _record(_enqueue(lib, handle, stream, clean, degraded, valid, cfg, valid_degraded=valid_degraded))


def cepstra(wav, valid=None, n_coef=13, variant="pwg"):
    """wav: device tensor [n] / [B, n] / [B, 1, n] -> [B, 1 + n // 256, n_coef] device float32.  valid: [B] sample counts of a padded
    batch; what lies behind them is not read, and the rows behind an item's own frames are zero.  Runs on the current stream, on the
    per-device handle of the operators (lvc_op)."""
    if variant not in VARIANTS:
        raise ValueError(f"mcd: variant must be 'pwg' or 'tacotron', got {variant!r}")
    return _cepstra(*_wave.default_handle(wav), wav, valid, n_coef, variant)


def dtw(a, b, frames_a=None, frames_b=None, align=False):
    """a [B, Ta, D], b [B, Tb, D] device float32 -> record of the B alignments (one synchronisation); align=True: (record, [B, Ta] int32
    on the device).  frames_a, frames_b: [B] row counts of padded batches; what lies behind them is not read."""
    return _dtw(*_wave.default_handle(a), a, b, frames_a, frames_b, align)


def measure(clean, degraded, valid=None, valid_degraded=None, **cfg):
    """clean [B, nc], degraded [B, nd] device tensors -> record of the B pairs (one synchronisation).  valid, valid_degraded: [B] sample
    counts of the padded batches (valid_degraded=None: valid counts for both).  cfg: n_coef, variant.  FastDiff.mcd uses the module's own
    handle."""
    return _measure(*_wave.default_handle(clean), clean, degraded, valid, cfg, valid_degraded=valid_degraded)
