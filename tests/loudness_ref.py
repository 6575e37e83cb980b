"""The float64 oracle of the loudness meter (include/fastdiff_hip_ext.h: "BS.1770 loudness"): pyloudnorm.Meter(rate) with its defaults
for one channel and pyloudnorm.normalize.loudness, restated from their published definitions in numpy + scipy.signal.lfilter
(pyloudnorm is not in the build image).  Shared by tests/test_loudness.py and tools/loudness_probe.py; not a fallback of the library."""
import numpy as np
from scipy.signal import lfilter

OK, SHORT, SILENT, CLIPPED = 0, 1, 2, 3
T_G, STEP = 0.4, 0.25


def design(rate):
    """(b, a) of the high shelf and of the high pass, each divided by a0: RBJ forms, w0 = 2 pi fc / rate, alpha = sin w0 / (2 Q)."""
    G, Q, fc = 4.0, 1.0 / np.sqrt(2.0), 1500.0
    A = 10.0 ** (G / 40.0)
    w0 = 2.0 * np.pi * (fc / rate)
    alpha = np.sin(w0) / (2.0 * Q)
    c, s = np.cos(w0), 2.0 * np.sqrt(A) * alpha
    b = np.array([A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s)])
    a = np.array([(A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s])
    shelf = (b / a[0], a / a[0])
    Q, fc = 0.5, 38.0
    w0 = 2.0 * np.pi * (fc / rate)
    alpha = np.sin(w0) / (2.0 * Q)
    c = np.cos(w0)
    b = np.array([(1 + c) / 2, -(1 + c), (1 + c) / 2])
    a = np.array([1 + alpha, -2 * c, 1 - alpha])
    return shelf, (b / a[0], a / a[0])


def coef10(rate):
    """shelf b0 b1 b2 a1 a2, high pass b0 b1 b2 a1 a2: the order of fd_loudness_design."""
    (b1, a1), (b2, a2) = design(rate)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def blocks(n, rate):
    """nb = int(round((T - T_g) / (T_g step)) + 1) (numpy's round: half to even); 0 where pyloudnorm raises (n < int(T_g rate))."""
    if n < int(T_G * rate):
        return 0
    T = n / rate
    return int(np.round((T - T_G) / (T_G * STEP)) + 1)


def block_powers(x, rate):
    """z_j of every block: the K-weighted signal's sum of squares over [int(T_g (j step) rate), int(T_g (j step + 1) rate)) cut to n,
    divided by T_g rate."""
    x = np.asarray(x, np.float64).reshape(-1)
    y = x
    for b, a in design(rate):
        y = lfilter(b, a, y)
    nb = blocks(x.shape[0], rate)
    z = np.zeros(nb)
    for j in range(nb):
        lo, hi = int(T_G * (j * STEP) * rate), int(T_G * (j * STEP + 1) * rate)
        z[j] = np.sum(np.square(y[lo:hi])) / (T_G * rate)
    return z


def measure(x, rate, target=None):
    """dict(lufs, gain, peak, blocks, gated, status, margin) of one utterance, float32 samples; margin: the smallest distance in LU
    of a block's loudness from either gate (inf if there is none to compare).  With a target: the gain that normalises to it
    (1 / peak and CLIPPED where peak gain > 1); without: gain 1."""
    x32 = np.asarray(x, np.float32).reshape(-1)
    peak = np.float32(np.abs(x32).max()) if x32.size else np.float32(0)
    r = dict(lufs=-np.inf, gain=np.float32(1), peak=peak, blocks=0, gated=0, status=SHORT, margin=np.inf)
    if x32.shape[0] < int(T_G * rate):
        return r
    z = block_powers(x32, rate)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    r["blocks"], r["status"] = z.shape[0], SILENT
    J = l >= -70.0
    r["margin"] = float(np.abs(l[np.isfinite(l)] + 70.0).min()) if np.isfinite(l).any() else np.inf
    if not J.any():
        return r
    gamma = -0.691 + 10.0 * np.log10(np.mean(z[J])) - 10.0
    r["margin"] = min(r["margin"], float(np.abs(l[np.isfinite(l)] - gamma).min()))
    Jp = (l > gamma) & (l > -70.0)
    if not Jp.any():
        return r
    r["gated"], r["status"] = int(Jp.sum()), OK
    r["lufs"] = float(-0.691 + 10.0 * np.log10(np.mean(z[Jp])))
    if target is not None:
        g = 10.0 ** ((target - r["lufs"]) / 20.0)
        if float(peak) * g > 1.0:
            r["status"], r["gain"] = CLIPPED, np.float32(1) / peak
        else:
            r["gain"] = np.float32(g)
    return r


def normalize(x, rate, target, out="float"):
    """(output, record): float32 x gain, or int16 (int16)(float32(x) float32(gain) 32767f); SHORT / SILENT / CLIPPED utterances as the
    library defines them (float: unchanged / unchanged / x / peak; int16: the peak epilogue, x / peak * 32767 truncated)."""
    x32 = np.asarray(x, np.float32).reshape(-1)
    r = measure(x32, rate, target)
    if out == "float":
        y = x32 * r["gain"] if r["status"] == OK else (x32 / r["peak"] if r["status"] == CLIPPED else x32.copy())
        return y.astype(np.float32), r
    v = x32 * r["gain"] if r["status"] == OK else x32 / r["peak"]
    return (v.astype(np.float32) * np.float32(32767.0)).astype(np.int16), r
