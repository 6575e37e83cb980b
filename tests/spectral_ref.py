"""The float64 oracle of the multi-resolution STFT distances (include/fastdiff_hip_ext.h: "Multi-resolution STFT distances", steps 1-7):
the header's text restated in numpy.  tests/test_spectral.py confirms its magnitudes with torch.stft in float64 on the CPU.  Shared by
the tests; not a fallback of the library."""
import numpy as np

OK, SHORT = 0, 1
MAX_RES = 4
DEFAULT_RES = ((512, 50, 240), (1024, 120, 600), (2048, 240, 1200))
DEFAULT_FLOOR = 1e-7
DB_PER_NEPER = 20.0 / np.log(10.0)


def frames(n, hop):
    return 1 + n // hop


def accepted(res=DEFAULT_RES, floor=DEFAULT_FLOOR):
    """Whether the header accepts the configuration."""
    if not 1 <= len(res) <= MAX_RES or not (floor > 0 and np.isfinite(floor)):
        return False
    return all(nfft in (512, 1024, 2048) and 2 <= win <= nfft and 16 <= hop <= nfft for nfft, hop, win in res)


def window(nfft, win):
    """Step 3: the periodic Hann window of `win` samples at offset (nfft - win) // 2 of the frame."""
    w = np.zeros(nfft)
    off = (nfft - win) // 2
    w[off: off + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def power(s, nfft, hop, win):
    """Steps 1-4 without the floor: re^2 + im^2 [F, nfft / 2 + 1] of one signal with n > nfft / 2."""
    s = np.asarray(s, np.float64)
    n = len(s)
    assert n > nfft // 2
    p = np.arange(frames(n, hop))[:, None] * hop - nfft // 2 + np.arange(nfft)[None, :]
    p = np.where(p < 0, -p, np.where(p >= n, 2 * (n - 1) - p, p))
    spec = np.fft.rfft(s[p] * window(nfft, win)[None, :], axis=1)
    return spec.real ** 2 + spec.imag ** 2


def magnitudes(s, nfft, hop, win, floor=DEFAULT_FLOOR):
    return np.sqrt(np.maximum(power(s, nfft, hop, win), floor))


def measure(x, y, res=DEFAULT_RES, floor=DEFAULT_FLOOR, detail=False):
    """x the recording, y the vocoded waveform, [n] -> the record: sc, logmag, lsd [MAX_RES] (NaN beyond len(res) or when SHORT), mr_sc,
    mr_logmag, lsd_db, frames [MAX_RES], n_res, status; detail adds floored = the share of the bins of x and y at the floor."""
    assert accepted(res, floor) and len(x) == len(y)
    n = len(x)
    out = {"sc": np.full(MAX_RES, np.nan), "logmag": np.full(MAX_RES, np.nan), "lsd": np.full(MAX_RES, np.nan), "mr_sc": np.nan,
           "mr_logmag": np.nan, "lsd_db": np.nan, "frames": np.zeros(MAX_RES, np.int32), "n_res": len(res), "status": OK}
    for r, (nfft, hop, win) in enumerate(res):
        out["frames"][r] = frames(n, hop)
    if n <= max(nfft // 2 for nfft, _, _ in res):
        out["status"] = SHORT
        return out
    at_floor = total = 0
    for r, (nfft, hop, win) in enumerate(res):
        px, py = power(x, nfft, hop, win), power(y, nfft, hop, win)
        at_floor += int((px <= floor).sum()) + int((py <= floor).sum())
        total += 2 * px.size
        X, Y = np.sqrt(np.maximum(px, floor)), np.sqrt(np.maximum(py, floor))
        d = np.log(X) - np.log(Y)
        out["sc"][r] = np.sqrt(((X - Y) ** 2).sum() / (X ** 2).sum())
        out["logmag"][r] = np.abs(d).mean()
        out["lsd"][r] = np.sqrt(((DB_PER_NEPER * d) ** 2).mean(axis=1)).mean()
    k = len(res)
    out["mr_sc"], out["mr_logmag"], out["lsd_db"] = out["sc"][:k].mean(), out["logmag"][:k].mean(), out["lsd"][:k].mean()
    if detail:
        out["floored"] = at_floor / total
    return out
