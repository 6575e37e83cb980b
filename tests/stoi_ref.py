"""The float64 oracle of STOI and ESTOI (include/fastdiff_hip_ext.h: "STOI and ESTOI", steps 1-9): the header's text restated in numpy,
with resample.resample_host for step 1.  pystoi is not in the build image, so the header defines the measurement (pystoi's conventions
as recalled, not as checked) and this file follows the header.  Shared by tests/test_stoi.py; not a fallback of the library."""
import numpy as np

OK, SHORT, SILENT = 0, 1, 2
RATE, FRAME, HOP, NFFT, BANDS, SEG = 10000, 256, 128, 512, 15, 30
EPS = float(np.finfo(np.float64).eps)                       # 2^-52
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(FRAME) + 1.0) / (FRAME + 1.0))      # hanning(258)[1:-1]


def bands():
    """(lo, hi): band j sums the bins [lo[j], hi[j]) -- the bins nearest to 150 * 2^((2j -+ 1) / 6) Hz on the grid k * 10000 / 512."""
    f = np.arange(NFFT // 2 + 1) * (RATE / NFFT)
    j = np.arange(BANDS)
    fl, fr = 150.0 * 2.0 ** ((2 * j - 1) / 6.0), 150.0 * 2.0 ** ((2 * j + 1) / 6.0)
    lo = [int(np.argmin((f - v) ** 2)) for v in fl]
    hi = [int(np.argmin((f - v) ** 2)) for v in fr]
    return lo, hi


def frames(n):
    """F0 = len(range(0, n - 256, 128))."""
    return len(range(0, n - FRAME, HOP))


def _frames_of(x):
    return np.array([WINDOW * x[i: i + FRAME] for i in range(0, len(x) - FRAME, HOP)]).reshape(-1, FRAME)


def _overlap_add(fr):
    out = np.zeros(HOP * (len(fr) - 1) + FRAME)
    for k, f in enumerate(fr):
        out[k * HOP: k * HOP + FRAME] += f
    return out


def _band_amplitudes(x):
    """[15, M] of the silence-free signal x."""
    fr = _frames_of(x)
    P = np.abs(np.fft.rfft(fr, n=NFFT, axis=1)) ** 2       # [M, 257]
    lo, hi = bands()
    return np.sqrt(np.array([P[:, a:b].sum(axis=1) for a, b in zip(lo, hi)]))


def _row_col_normalize(s):
    """s [J, 15, 30]: every row (a band over time), then every column (a frame over bands): mean removed, divided by norm + eps."""
    s = s - s.mean(axis=2, keepdims=True)
    s = s / (np.linalg.norm(s, axis=2, keepdims=True) + EPS)
    s = s - s.mean(axis=1, keepdims=True)
    return s / (np.linalg.norm(s, axis=1, keepdims=True) + EPS)


def measure(x, y, rate=RATE, detail=False):
    """x clean, y degraded, [n] -> {"stoi", "estoi", "frames", "kept", "segments", "status", "margin"}; margin = the smallest
    |10 log10(E_i / (1e-4 max E))| over the frames in dB (inf where there is nothing to decide).  detail: also "clipped", the fraction
    of (segment, band, frame) entries on which step 7's clip acts."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.shape == y.shape and x.ndim == 1
    if rate != RATE:
        from fastdiff_amd import resample
        x = resample.resample_host(x.astype(np.float32), rate, RATE).astype(np.float64).reshape(-1)
        y = resample.resample_host(y.astype(np.float32), rate, RATE).astype(np.float64).reshape(-1)
    nan = float("nan")
    out = {"stoi": nan, "estoi": nan, "frames": frames(len(x)), "kept": 0, "segments": 0, "status": SHORT, "margin": float("inf")}
    if out["frames"] == 0:
        return out
    xf, yf = _frames_of(x), _frames_of(y)
    E = (xf ** 2).sum(axis=1)
    if E.max() == 0.0:
        out["status"] = SILENT
        return out
    thr = 1e-4 * E.max()
    with np.errstate(divide="ignore"):
        out["margin"] = float(np.abs(10.0 * np.log10(E / thr)).min())
    mask = E > thr
    K = int(mask.sum())
    out["kept"] = K
    if K < SEG + 1:
        return out
    X, Y = _band_amplitudes(_overlap_add(xf[mask])), _band_amplitudes(_overlap_add(yf[mask]))
    M = X.shape[1]
    assert M == K - 1
    J = M - (SEG - 1)
    xs = np.array([X[:, s: s + SEG] for s in range(J)])    # [J, 15, 30]
    ys = np.array([Y[:, s: s + SEG] for s in range(J)])
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yn = ys * c
    clip = xs * CLIP
    yp = np.minimum(yn, clip)
    xm = xs - xs.mean(axis=2, keepdims=True)
    ym = yp - yp.mean(axis=2, keepdims=True)
    xm = xm / (np.linalg.norm(xm, axis=2, keepdims=True) + EPS)
    ym = ym / (np.linalg.norm(ym, axis=2, keepdims=True) + EPS)
    out["stoi"] = float((xm * ym).sum() / (BANDS * J))
    out["estoi"] = float((_row_col_normalize(xs) * _row_col_normalize(ys)).sum() / (SEG * J))
    out["segments"], out["status"] = J, OK
    if detail:
        out["clipped"] = float((yn > clip).mean())
    return out
