"""What the waveform tools (resample, loudness, stoi, pitch, FastDiff.peak_normalize_int16) share in front of and behind their C calls."""
import ctypes as ct

import torch


def rows(t, who, what="wav"):
    """A device tensor [n] / [B, n] / [B, 1, n] -> (it as contiguous float32 of B rows, B, L = the samples of a row); an empty one is
    refused."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{who}: a tensor on the HIP device is expected (there is no CPU path)")
    t = t.contiguous().float()
    if t.dim() == 1:
        t = t.unsqueeze(0)
    B = t.shape[0]
    L = t.numel() // max(B, 1)
    if B < 1 or L < 1:
        raise ValueError(f"{who}: empty {what} of shape {list(t.shape)}")
    return t, B, L


def counts(valid, B, who):
    """The [B] counts of a padded batch as the C calls take them; None stays None."""
    if valid is None:
        return None
    if len(valid) != B:
        raise ValueError(f"{who}: valid has {len(valid)} entries for {B} rows")
    return (ct.c_int64 * B)(*[int(v) for v in valid])


def records(rec, dtype, fields):
    """The device records [B, itemsize] uint8 -> dict of numpy arrays (one synchronising copy)."""
    r = rec.cpu().numpy().view(dtype).reshape(-1)
    return {k: r[k].copy() for k in fields}


def default_handle(t):
    """(lib, handle, stream) of the module-level functions: the per-device handle of the operators (lvc_op), the current stream."""
    from . import lvc_op
    lib, h = lvc_op._handle(t.device)
    return lib, h, lvc_op._stream(t.device)
