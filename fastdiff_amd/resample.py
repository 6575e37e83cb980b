"""Sample-rate conversion on the device: recordings of any rate, sample type and channel count in, waveforms of any rate out.

The reference resamples silently at the first line of its front-end: `librosa.core.load(wav_path, sr=sample_rate)`
(data_gen/tts/data_gen_utils.py:111, :40-49; vocoders/pwg.py:132) mixes a recording down to mono and brings it to the model's rate.
Here that is one kernel launch (fd_resample, include/fastdiff_hip_ext.h) from the file's own samples to float mono:

    up / down = sr_out / sr_in reduced, q = max(up, down), half = ZEROS q
    g[k] = sinc(ROLLOFF (k - half) / q) kaiser(k; 2 half + 1, BETA), divided by its sum      (scipy.signal.firwin(2 half + 1, ROLLOFF / q,
                                                                                              window=("kaiser", BETA)))
    y[i] = sum_j x[j] h[i down - j up + half],  h = float32(up g),  n_out = ceil(n up / down) (scipy.signal.resample_poly(x, up, down,
                                                                                              window=g), sample for sample)

ZEROS, ROLLOFF and BETA are the parameters resampy publishes for "kaiser_best", the filter librosa used by default at the reference's
time; neither package is needed or compared against (resampy interpolates a tabulated filter: the same design, not the same bits).

    design(sr_in, sr_out)        the prototype g in float64 numpy -- the twin of the library's host code (csrc/fd_resample.h)
    taps(sr_in, sr_out)          the float32 h the kernel multiplies with, from the library
    out_len(n, sr_in, sr_out)    ceil(n up / down)
    resample(x, sr_in, sr_out, valid=None, channels=1)      device tensors float32 / int16 / int32 / uint8 -> float32 [B, out_len(n)]
    resample_host(x, sr_in, sr_out)                          the definition in float64 numpy (inspection and tests, not a fallback)
"""
import ctypes as ct
from math import gcd

import numpy as np
import torch

from . import _capi, _wave

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
MAX_RATIO = _capi.FD_RESAMPLE_MAX_RATIO
_FORMATS = {torch.float32: _capi.FD_PCM_F32, torch.int16: _capi.FD_PCM_S16, torch.int32: _capi.FD_PCM_S32, torch.uint8: _capi.FD_PCM_U8}


def ratio(sr_in, sr_out):
    """(up, down, half, K): the reduced ratio, half = ZEROS max(up, down) and the taps per output K = ceil((2 half + 1) / up)."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"resample: sample rates {sr_in} -> {sr_out}")
    d = gcd(sr_in, sr_out)
    up, down = sr_out // d, sr_in // d
    if max(up, down) > MAX_RATIO:
        raise NotImplementedError(f"resample: {sr_in} -> {sr_out} Hz reduces to {up}/{down}; ratios up to {MAX_RATIO} are supported")
    half = ZEROS * max(up, down)
    return up, down, half, -(-(2 * half + 1) // up)


def design(sr_in, sr_out):
    """The prototype low-pass g [2 half + 1] in float64: the windowed sinc above, divided by its sum."""
    up, down, half, _ = ratio(sr_in, sr_out)
    m = np.arange(-half, half + 1, dtype=np.float64)
    g = np.sinc(ROLLOFF * m / max(up, down)) * np.kaiser(2 * half + 1, BETA)
    return g / g.sum()


def taps(sr_in, sr_out):
    """(h float32 [2 half + 1], up, down, half) as the library computes them (fd_resample_taps): h = up g rounded once."""
    lib = _capi.load()
    up, down, half = ct.c_int(), ct.c_int(), ct.c_int()
    n = lib.fd_resample_taps(int(sr_in), int(sr_out), None, 0, ct.byref(up), ct.byref(down), ct.byref(half))
    _capi.check(lib, None, n, f"fd_resample_taps({sr_in}, {sr_out})")
    h = np.empty(n, np.float32)
    _capi.check(lib, None, lib.fd_resample_taps(int(sr_in), int(sr_out), h.ctypes.data, n, None, None, None), "fd_resample_taps")
    return h, up.value, down.value, half.value


def out_len(n, sr_in, sr_out):
    """Samples that `n` input samples become: ceil(n up / down) (fd_resample_out_len)."""
    lib = _capi.load()
    r = lib.fd_resample_out_len(int(n), int(sr_in), int(sr_out))
    if r == _capi.FD_ERR_UNSUPPORTED:
        raise NotImplementedError(f"resample: {sr_in} -> {sr_out} Hz does not reduce to a ratio within {MAX_RATIO}")
    if r < 0:
        raise ValueError(f"resample: out_len({n}, {sr_in}, {sr_out})")
    return int(r)


def resample_host(x, sr_in, sr_out, h=None, rows=4096):
    """The definition in float64 numpy: y[i] = sum_j x[j] h[i down - j up + half] over a 1-D signal, `h` = float64(up * design())
    unless given (e.g. taps()[0]).  O(n_out K) memory-bounded by `rows` outputs at a time."""
    up, down, half, K = ratio(sr_in, sr_out)
    x = np.asarray(x, np.float64).reshape(-1)
    h = up * design(sr_in, sr_out) if h is None else np.asarray(h, np.float64)
    n = x.shape[0]
    n_out = -(-n * up // down)
    y = np.zeros(n_out, np.float64)
    m = np.arange(K, dtype=np.int64)
    for i0 in range(0, n_out, rows):
        a = np.arange(i0, min(i0 + rows, n_out), dtype=np.int64) * down + half
        j = (a // up)[:, None] - (K - 1) + m[None, :]              # ascending inputs of every output
        t = a[:, None] - j * up                                   # their tap
        ok = (j >= 0) & (j < n) & (t >= 0) & (t <= 2 * half)
        y[i0: i0 + a.shape[0]] = np.where(ok, x[np.clip(j, 0, n - 1)] * h[np.clip(t, 0, 2 * half)], 0.0).sum(axis=1)
    return y


def _run(lib, handle, stream, x, sr_in, sr_out, valid, channels):
    """fd_resample on a device tensor: [n] / [B, n] (channels = 1) or [n, C] / [B, n, C] (interleaved channels) -> [B, out_len(n)]."""
    channels = int(channels)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("resample: a tensor on the HIP device is expected (there is no CPU path)")
    if x.dtype not in _FORMATS:
        raise ValueError(f"resample: unsupported sample type {x.dtype} (float32, int16, int32 or uint8)")
    if channels == 1:
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise ValueError(f"resample: expected [n] or [B, n], got shape {list(x.shape)}")
        x = x.unsqueeze(-1)
    else:
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[-1] != channels:
            raise ValueError(f"resample: expected [n, {channels}] or [B, n, {channels}], got shape {list(x.shape)}")
    B, n, C = x.shape
    if B < 1 or n < 1:
        raise ValueError(f"resample: empty input of shape {list(x.shape)}")
    if x.stride(2) != 1 or x.stride(1) != C or (B > 1 and x.stride(0) < n * C):      # rows may keep their own pitch
        x = x.contiguous()
    pitch = x.stride(0) if B > 1 else n * C
    n_out = out_len(n, sr_in, sr_out)
    y = torch.empty((B, n_out), device=x.device, dtype=torch.float32)
    varr = _wave.counts(valid, B, "resample")
    rc = lib.fd_resample(handle, x.data_ptr(), _FORMATS[x.dtype], C, B, n, pitch, varr, int(sr_in), int(sr_out), y.data_ptr(), n_out, stream)
    _capi.check(lib, handle, rc, "fd_resample")
    return y


def resample(x, sr_in, sr_out, valid=None, channels=1):
    """x: a device tensor [n] / [B, n], or with channels = C > 1 interleaved frames [n, C] / [B, n, C]; float32 as is, int16 / 32768,
    int32 / 2^31, uint8 (v - 128) / 128; the channels are averaged.  -> float32 [B, out_len(n)] at sr_out.
    valid (optional, [B] frame counts of a zero-padded batch): item b is resampled as if it were valid[b] frames long, and its row is 0
    behind out_len(valid[b]).  An item's result does not depend on the batch it is in.  Equal rates: conversion and down-mix only.
    Runs on the current stream, on the per-device handle of the operators (lvc_op); FastDiff.resample uses the module's own."""
    return _run(*_wave.default_handle(x), x, sr_in, sr_out, valid, channels)
