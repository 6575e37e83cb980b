"""Griffin-Lim on the device: the baseline vocoder, and the inverse STFT and magnitude-only reconstruction loop it is made of.

The reference registers GLLinear and GLMel next to FastDiff (vocoders/gl_linear.py, vocoders/gl_mel.py over utils/audio.py:35-63
griffin_lim and :123-158 griffin_lim_torch); every score of the bench (STOI, F0 errors, STFT distances, loudness) wants the same columns
for that baseline, run on the same mels.  Here it is one call (fd_griffin_lim, include/fastdiff_hip_ext.h, which defines the computation:
n_fft 1024, hop 256, the periodic Hann window, zero padding of 512 as the mel front-end frames a recording, frames t < lens[b] ->
256 (lens[b] - 1) samples; C_0 = A e^(i theta0), then n_iters times X = stft(y), C = A X / |X|, y = istft(C)).  n_iters = 0 with given
angles is the inverse STFT alone.

    samples(frames)              256 (frames - 1): the front-end's T = 1 + len // 256 read backwards
    default_iters()              60 (griffin_lim_iters, egs_bases/tts/base.yaml)
    pinv(filterbank, variant)    the pseudo-inverse [513, 80] of a filter bank [80, 513], float64 numpy.linalg.pinv rounded to float32,
                                 cached per variant until the bank changes
    mel_to_linear(mel, pinv, variant="pwg")                       -> amplitudes [B, 513, T]
    mel_to_linear_nnls(mel, bank, pinv, variant="pwg", lens=None, n_iters=128, return_record=False)      -> amplitudes [B, 513, T]
    nnls_default_iters()         128
    nnls_step_bound(bank)        L >= lambda_max(bank bank^T): the step of the non-negative inversion is 1 / L
    griffin_lim(amp, lens=None, n_iters=60, angles=None, seed=0, stream_ids=None, return_record=False)   -> wav [B, 256 (T - 1)]
    STATUS, NNLS_STATUS          names of the records' status values

mel_to_linear is utils/audio.py:91-95 _mel_to_linear: max(1e-10, pinv(basis) @ g(mel)), g = 10^x for "pwg" mels and e^x for
"tacotron" ones: the pseudo-inverse, and the default inversion everywhere.  mel_to_linear_nnls is the non-negative least squares that
GLMel's librosa.feature.inverse.mel_to_stft runs (librosa.util.nnls, an L-BFGS-B solve per block): per frame min || bank x - g(mel) ||,
x >= 0, started at the clipped pseudo-inverse and solved by n_iters accelerated projected-gradient steps of fixed size in one fused
kernel (fd_mel_to_linear_nnls, which defines it), then floored at 1e-10 like the other.  n_iters = 0 is mel_to_linear bit for bit.
Its record: resid (float64: || bank amp - g || / || g || over the item's own frames, NaN unless OK), norm (|| g ||), frames, iters,
status (int32).  EMPTY: no frames; NONFINITE: a mel value is NaN or infinite or g overflows, the item's amplitudes are then all 1e-10.

A record is a dict of numpy arrays over the batch: sc (float64: || |stft(y)| - A || / || A || of the returned waveform, NaN unless OK),
norm (|| A ||), frames, samples, iters, status (int32).  SHORT: fewer than 2 frames; SILENT: every amplitude is 0; NONFINITE: an
amplitude is negative, infinite or NaN; the waveform of such an item is zeros.
"""
import ctypes as ct

import numpy as np
import torch

from . import _capi, _wave

NFFT, HOP, BINS, MELS = _capi.FD_GL_NFFT, _capi.FD_GL_HOP, _capi.FD_GL_BINS, 80
FRAME_TILE, MAX_ITERS, PHILOX_STREAM = _capi.FD_GL_FRAME_TILE, _capi.FD_GL_MAX_ITERS, _capi.FD_GL_PHILOX_STREAM
OK, SHORT, SILENT, NONFINITE = _capi.FD_GL_OK, _capi.FD_GL_SHORT, _capi.FD_GL_SILENT, _capi.FD_GL_NONFINITE
STATUS = {OK: "OK", SHORT: "SHORT", SILENT: "SILENT", NONFINITE: "NONFINITE"}
RECORD = _capi.record("fd_gl")
VARIANTS = {"pwg": _capi.FD_GL_PWG, "tacotron": _capi.FD_GL_TACOTRON}

NNLS_MAX_ITERS, NNLS_FRAME_TILE = _capi.FD_NNLS_MAX_ITERS, _capi.FD_NNLS_FRAME_TILE
NNLS_OK, NNLS_EMPTY, NNLS_NONFINITE = _capi.FD_NNLS_OK, _capi.FD_NNLS_EMPTY, _capi.FD_NNLS_NONFINITE
NNLS_STATUS = {NNLS_OK: "OK", NNLS_EMPTY: "EMPTY", NNLS_NONFINITE: "NONFINITE"}
NNLS_RECORD = _capi.record("fd_nnls")

_pinv_cache = {}      # variant -> (the bank's bytes, its pseudo-inverse)


def samples(frames):
    """Samples of `frames` frames (fd_gl_samples): 256 (frames - 1)."""
    r = _capi.load().fd_gl_samples(int(frames))
    if r < 0:
        raise ValueError(f"griffin_lim: samples({frames}): at least 2 frames")
    return int(r)


def default_iters():
    return int(_capi.load().fd_gl_default_iters())


def variant_id(variant):
    if variant not in VARIANTS:
        raise ValueError(f"griffin_lim: variant must be 'pwg' or 'tacotron', got {variant!r}")
    return VARIANTS[variant]


def pinv(filterbank, variant="pwg"):
    """The pseudo-inverse [513, 80] float32 of `filterbank` [80, 513]: numpy.linalg.pinv in float64, rounded once.  Cached per variant;
    computed again when the bank's values differ from the cached one's."""
    variant_id(variant)
    fb = np.ascontiguousarray(filterbank, dtype=np.float32)
    if fb.shape != (MELS, BINS):
        raise ValueError(f"griffin_lim: expected a filter bank [80, 513], got {list(fb.shape)}")
    key = fb.tobytes()
    hit = _pinv_cache.get(variant)
    if hit is None or hit[0] != key:
        P = np.ascontiguousarray(np.linalg.pinv(fb.astype(np.float64)).astype(np.float32))
        P.setflags(write=False)
        hit = _pinv_cache[variant] = (key, P)
    return hit[1]


def _mel_to_linear(lib, handle, stream, mel, P, variant):
    v = variant_id(variant)
    if not isinstance(mel, torch.Tensor) or not mel.is_cuda:
        raise ValueError("mel_to_linear: a tensor on the HIP device is expected (there is no CPU path)")
    mel = mel.contiguous().float()
    if mel.dim() == 2:
        mel = mel.unsqueeze(0)
    if mel.dim() != 3 or mel.shape[1] != MELS or mel.shape[2] < 1:
        raise ValueError(f"mel_to_linear: expected a mel [B, 80, T], got {list(mel.shape)}")
    P = np.ascontiguousarray(P, dtype=np.float32)
    if P.shape != (BINS, MELS):
        raise ValueError(f"mel_to_linear: expected a pseudo-inverse [513, 80], got {list(P.shape)}")
    B, _, T = mel.shape
    amp = torch.empty((B, BINS, T), device=mel.device, dtype=torch.float32)
    _capi.check(lib, handle, lib.fd_mel_to_linear(handle, mel.data_ptr(), B, T, P.ctypes.data, v, amp.data_ptr(), stream), "fd_mel_to_linear")
    return amp


def nnls_default_iters():
    return int(_capi.load().fd_nnls_default_iters())


def nnls_step_bound(filterbank):
    """L of fd_nnls_step_bound for a filter bank [80, 513]: 1.01 times the Rayleigh quotient of bank bank^T after 200 power iterations."""
    fb = np.ascontiguousarray(filterbank, dtype=np.float32)
    if fb.shape != (MELS, BINS):
        raise ValueError(f"griffin_lim: expected a filter bank [80, 513], got {list(fb.shape)}")
    lib, L = _capi.load(), ct.c_double()
    _capi.check(lib, None, lib.fd_nnls_step_bound(fb.ctypes.data, ct.byref(L)), "fd_nnls_step_bound")
    return float(L.value)


def _mel_to_linear_nnls(lib, handle, stream, mel, bank, P, variant, lens, n_iters, return_record):
    v = variant_id(variant)
    if not isinstance(mel, torch.Tensor) or not mel.is_cuda:
        raise ValueError("mel_to_linear_nnls: a tensor on the HIP device is expected (there is no CPU path)")
    mel = mel.contiguous().float()
    if mel.dim() == 2:
        mel = mel.unsqueeze(0)
    if mel.dim() != 3 or mel.shape[1] != MELS or mel.shape[2] < 1:
        raise ValueError(f"mel_to_linear_nnls: expected a mel [B, 80, T], got {list(mel.shape)}")
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    if bank.shape != (MELS, BINS):
        raise ValueError(f"mel_to_linear_nnls: expected a filter bank [80, 513], got {list(bank.shape)}")
    P = np.ascontiguousarray(P, dtype=np.float32)
    if P.shape != (BINS, MELS):
        raise ValueError(f"mel_to_linear_nnls: expected a pseudo-inverse [513, 80], got {list(P.shape)}")
    B, _, T = mel.shape
    amp = torch.empty((B, BINS, T), device=mel.device, dtype=torch.float32)
    rec = torch.empty((B, NNLS_RECORD.itemsize), device=mel.device, dtype=torch.uint8) if return_record else None
    rc = lib.fd_mel_to_linear_nnls(handle, mel.data_ptr(), B, T, _wave.counts(lens, B, "mel_to_linear_nnls"), bank.ctypes.data, P.ctypes.data, v,
                                   int(n_iters), amp.data_ptr(), None if rec is None else rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_mel_to_linear_nnls")
    return (amp, _wave.records(rec, NNLS_RECORD, NNLS_RECORD.names[:5])) if return_record else amp


def _amp(amp, angles):
    if not isinstance(amp, torch.Tensor) or not amp.is_cuda:
        raise ValueError("griffin_lim: a tensor on the HIP device is expected (there is no CPU path)")
    amp = amp.contiguous().float()
    if amp.dim() == 2:
        amp = amp.unsqueeze(0)
    if amp.dim() != 3 or amp.shape[1] != BINS:
        raise ValueError(f"griffin_lim: expected amplitudes [B, 513, T], got {list(amp.shape)}")
    if angles is not None:
        if not isinstance(angles, torch.Tensor) or angles.device != amp.device:
            raise ValueError("griffin_lim: angles must be a tensor on the amplitudes' device")
        angles = angles.contiguous().float()
        if angles.dim() == 2:
            angles = angles.unsqueeze(0)
        if angles.shape != amp.shape:
            raise ValueError(f"griffin_lim: angles {list(angles.shape)} do not match the amplitudes {list(amp.shape)}")
    return amp, angles


def _enqueue(lib, handle, stream, amp, lens, n_iters, angles, seed, stream_ids, wav=None, rec=None):
    """fd_griffin_lim on the stream -> (wav [B, 256 (T - 1)], the device records [B, 32] uint8); nothing synchronises."""
    amp, angles = _amp(amp, angles)
    B, _, T = amp.shape
    L = max(HOP * (T - 1), 0)
    if wav is None:
        wav = torch.empty((B, L), device=amp.device, dtype=torch.float32)
    if rec is None:
        rec = torch.empty((B, RECORD.itemsize), device=amp.device, dtype=torch.uint8)
    assert wav.is_cuda and wav.dtype == torch.float32 and wav.is_contiguous() and wav.shape == (B, L)
    assert rec.is_cuda and rec.dtype == torch.uint8 and rec.is_contiguous() and rec.numel() == B * RECORD.itemsize
    ids = None
    if stream_ids is not None:
        if len(stream_ids) != B:
            raise ValueError(f"griffin_lim: stream_ids has {len(stream_ids)} entries for {B} items")
        ids = (ct.c_uint64 * B)(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in stream_ids])
    rc = lib.fd_griffin_lim(handle, amp.data_ptr(), None if angles is None else angles.data_ptr(), B, T, _wave.counts(lens, B, "griffin_lim"),
                            int(n_iters), int(seed) & 0xFFFFFFFFFFFFFFFF, ids, wav.data_ptr(), L, rec.data_ptr(), stream)
    _capi.check(lib, handle, rc, "fd_griffin_lim")
    return wav, rec


def _record(rec):
    return _wave.records(rec, RECORD, RECORD.names)


def _run(lib, handle, stream, amp, lens, n_iters, angles, seed, stream_ids, return_record):
    wav, rec = _enqueue(lib, handle, stream, amp, lens, n_iters, angles, seed, stream_ids)
    return (wav, _record(rec)) if return_record else wav


def mel_to_linear(mel, pinv_513x80, variant="pwg"):
    """mel [B, 80, T] on the device, the pseudo-inverse [513, 80] (pinv()) -> amplitudes [B, 513, T]: max(1e-10, P @ g(mel)).  Runs on
    the current stream, on the per-device handle of the operators (lvc_op); FastDiff.mel_to_linear uses the module's own and its bank."""
    return _mel_to_linear(*_wave.default_handle(mel), mel, pinv_513x80, variant)


def mel_to_linear_nnls(mel, bank, pinv_513x80, variant="pwg", lens=None, n_iters=128, return_record=False):
    """mel [B, 80, T] on the device, the filter bank [80, 513] and its pseudo-inverse [513, 80] (pinv()) -> amplitudes [B, 513, T]: the
    non-negative least-squares inversion (the module's text above), n_iters steps from max(0, P @ g(mel)).  lens: [B] frame counts of a
    padded batch; frames behind them are not read and come back as 1e-10.  return_record: (amp, record): one synchronisation; without
    it nothing synchronises.  Runs on the current stream, on the per-device handle of the operators."""
    return _mel_to_linear_nnls(*_wave.default_handle(mel), mel, bank, pinv_513x80, variant, lens, n_iters, return_record)


def griffin_lim(amp, lens=None, n_iters=60, angles=None, seed=0, stream_ids=None, return_record=False):
    """amp [B, 513, T] on the device -> wav [B, 256 (T - 1)] (and the record: one synchronisation).  lens: [B] frame counts of a padded
    batch; item b fills its first 256 (lens[b] - 1) samples, the rest of its row is 0.  angles: the starting phase [B, 513, T]; None: Philox
    angles keyed on (seed, stream_ids[b] or b, frame, bin).  Runs on the current stream, on the per-device handle of the operators."""
    return _run(*_wave.default_handle(amp), amp, lens, n_iters, angles, seed, stream_ids, return_record)
