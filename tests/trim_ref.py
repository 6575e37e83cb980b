"""The float64 restatement of the silence trimmer (include/fastdiff_hip_ext.h: "Cutting long silences", steps 1-7), in numpy.  Written
from the method's text, not from the library's code and not from the reference's: tests/test_trim.py compares the device against it,
and compares ITS smoothing and dilation with the reference's formulation (a cumulative-sum moving average followed by np.round;
scipy.ndimage.binary_dilation).
"""
import numpy as np

OK, SILENT, EMPTY = 0, 1, 2
SPEECH, SMOOTH, KEEP = 1, 2, 4
E_FLOOR = 1e-20


def windows(n, rate, window_ms=30):
    """(W, M): W = window_ms rate / 1000, M = max(1, n / W), integer divisions."""
    W = window_ms * rate // 1000
    return W, max(1, n // W)


def bounds(n, rate, window_ms=30):
    """[(lo, hi)] of the M windows: window w < M - 1 covers [w W, (w + 1) W), the last one takes the tail."""
    W, M = windows(n, rate, window_ms)
    return [(w * W, (w + 1) * W if w < M - 1 else n) for w in range(M)]


def levels(x, rate, window_ms=30):
    """level_w = 10 log10(max(mean((x - mean x)^2), 1e-20)); NaN for a window with a sample that is not finite."""
    x = np.asarray(x, np.float32)
    out = []
    for lo, hi in bounds(len(x), rate, window_ms):
        seg = x[lo:hi].astype(np.float64)
        if not np.all(np.isfinite(seg)):
            out.append(np.nan)
            continue
        m = seg.mean()
        out.append(10.0 * np.log10(max(np.mean((seg - m) ** 2), E_FLOOR)))
    return np.asarray(out, np.float64)


def smooth(speech, A=8):
    """c_w = the flags among w - (A - 1) / 2 .. w + A / 2 (0 outside); smooth_w = 2 c_w > A."""
    s = np.asarray(speech, bool)
    M = len(s)
    out = np.zeros(M, bool)
    for w in range(M):
        c = sum(1 for v in range(w - (A - 1) // 2, w + A // 2 + 1) if 0 <= v < M and s[v])
        out[w] = 2 * c > A
    return out


def dilate(sm, G=12):
    """keep_w = any smooth_v with |v - w| <= G / 2."""
    sm = np.asarray(sm, bool)
    M = len(sm)
    return np.asarray([bool(sm[max(0, w - G // 2): min(M, w + G // 2 + 1)].any()) for w in range(M)], bool)


def keep_mask(speech, A=8, G=12, mode="long"):
    sm = smooth(speech, A)
    keep = dilate(sm, G)
    if mode == "edges" and keep.any():
        idx = np.flatnonzero(keep)
        keep[idx[0]: idx[-1] + 1] = True
    return sm, keep


def trim(x, rate=22050, window_ms=30, top_db=40.0, floor_db=-70.0, A=8, G=12, mode="long"):
    """One utterance (float32 [n]) -> dict: out (float32 [n_out]), n_out, windows, speech, kept_windows, nonfinite, status, peak_db,
    threshold_db, levels [M], flags [M] (uint8), margin_db = the smallest |level - threshold| over the windows that have a level."""
    x = np.asarray(x, np.float32)
    n = len(x)
    if n == 0:
        return dict(out=x[:0], n_out=0, windows=0, speech=0, kept_windows=0, nonfinite=0, status=EMPTY, peak_db=-np.inf, threshold_db=floor_db,
                    levels=np.zeros(0), flags=np.zeros(0, np.uint8), margin_db=np.inf)
    lv = levels(x, rate, window_ms)
    has = ~np.isnan(lv)
    peak = lv[has].max() if has.any() else -np.inf
    thr = max(peak - top_db, floor_db)
    speech = np.zeros(len(lv), bool)
    speech[has] = lv[has] > thr
    sm, keep = keep_mask(speech, A, G, mode)
    take = np.zeros(n, bool)
    for (lo, hi), k in zip(bounds(n, rate, window_ms), keep):
        take[lo:hi] = k
    out = x[take]
    flags = (speech * SPEECH + sm * SMOOTH + keep * KEEP).astype(np.uint8)
    return dict(out=out, n_out=len(out), windows=len(lv), speech=int(speech.sum()), kept_windows=int(keep.sum()), nonfinite=int((~has).sum()),
                status=OK if keep.any() else SILENT, peak_db=peak, threshold_db=thr, levels=lv, flags=flags,
                margin_db=float(np.abs(lv[has] - thr).min()) if has.any() else np.inf)
