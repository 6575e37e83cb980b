"""The float64 oracle of the F0 tracker and the pitch scores (include/fastdiff_hip_ext.h: "F0 tracking", steps 1-5 and the record): the
header's text restated in numpy.  Praat, WORLD and librosa are not in the build image, so the header defines the measurement (YIN, de
Cheveigne and Kawahara 2002) and this file follows the header.  Shared by tests/test_pitch.py; not a fallback of the library.

track(x, ..., sums="float32") is the CPU emulation of the device's split: d(tau) in float32 with the kernel's four accumulators, the rest
in float64."""
import numpy as np

OK, SHORT, UNVOICED = 0, 1, 2
MAX_LAGS = 1024
DEFAULTS = dict(rate=22050, hop=256, win=1024, f0_min=80.0, f0_max=750.0, threshold=0.15)


def config(**cfg):
    c = dict(DEFAULTS)
    c.update(cfg)
    return c


def lags(**cfg):
    """(tau_min, tau_max), or None for a configuration the header refuses."""
    c = config(**cfg)
    if c["rate"] < 1 or not c["f0_min"] > 0 or not c["f0_max"] > 0:
        return None
    tau_min, tau_max = int(np.floor(c["rate"] / c["f0_max"])), int(np.ceil(c["rate"] / c["f0_min"]))
    if tau_min < 2 or tau_max <= tau_min or tau_max + 2 > MAX_LAGS or c["win"] < 64 or c["win"] > 2048 or c["hop"] < 1:
        return None
    if not 0.0 < c["threshold"] < 1.0:
        return None
    return tau_min, tau_max


def frames(n, hop=256):
    return n // hop


def _difference(seg, win, L, sums):
    """d(tau), tau = 0 .. L - 1, of one frame's span of samples.  float64: exact products, numpy's pairwise sums.  float32: the kernel's
    order -- accumulator j mod 4 takes fma((a - b), (a - b), acc), then (a0 + a1) + (a2 + a3)."""
    idx = np.arange(win)[None, :] + np.arange(L)[:, None]
    if sums == "float64":
        e = seg[None, :win] - seg[idx]
        return (e * e).sum(axis=1)
    s32 = seg.astype(np.float32)
    e = (s32[None, :win] - s32[idx]).astype(np.float64)      # the float32 difference, exactly
    sq = e * e                                               # exact in float64 (24 x 24 bits)
    acc = np.zeros((4, L), np.float32)
    for j in range(win):
        acc[j & 3] = (acc[j & 3].astype(np.float64) + sq[:, j]).astype(np.float32)      # one rounding to float32 (the double rounding through float64 is rare and tiny)
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])).astype(np.float64)


def track(x, detail=False, sums="float64", **cfg):
    """x: [n] -> (f0 [F], aper [F]) in float64; with detail=True a dict that also holds dprime [F, L], k0, k [F] (-1 where unvoiced),
    m_thr and m_desc [F]."""
    c = config(**cfg)
    tau_min, tau_max = lags(**c)
    L, win, hop, thr = tau_max + 2, c["win"], c["hop"], c["threshold"]
    span = win + tau_max + 1
    x = np.asarray(x, np.float64)
    n = len(x)
    F = n // hop
    f0, aper = np.zeros(F), np.ones(F)
    dps, k0s, ks, m_thr, m_desc = np.ones((F, L)), -np.ones(F, int), -np.ones(F, int), np.zeros(F), np.full(F, np.inf)
    taus = np.arange(L)
    for i in range(F):
        s = i * hop + hop // 2 - span // 2
        seg = np.zeros(span)
        lo, hi = max(s, 0), min(s + span, n)
        if hi > lo:
            seg[lo - s: hi - s] = x[lo: hi]
        d = _difference(seg, win, L, sums)
        cum = np.cumsum(d[1:])
        dp = np.ones(L)
        nz = cum > 0
        dp[1:][nz] = d[1:][nz] * taus[1:][nz] / cum[nz]
        dps[i] = dp
        rng = dp[tau_min: tau_max + 1]
        below = np.nonzero(rng < thr)[0]
        if len(below) == 0:
            aper[i] = rng.min()
            m_thr[i] = np.abs(rng - thr).min()
            continue
        k0 = k = tau_min + int(below[0])
        while k + 1 <= tau_max and dp[k + 1] < dp[k]:
            k += 1
        k0s[i], ks[i] = k0, k
        m_thr[i] = np.abs(dp[tau_min: k0 + 1] - thr).min()
        m_desc[i] = np.abs(dp[k0 + 1: k + 2] - dp[k0: k + 1]).min()
        a, b, cc = dp[k - 1], dp[k], dp[k + 1]
        den = a - 2 * b + cc
        off = 0.5 * (a - cc) / den if den > 0 else 0.0
        off = min(max(off, -1.0), 1.0)
        f0[i] = c["rate"] / (k + off)
        aper[i] = b
    if not detail:
        return f0, aper
    return {"f0": f0, "aper": aper, "dprime": dps, "k0": k0s, "k": ks, "m_thr": m_thr, "m_desc": m_desc}


def compare(f_ref, f_deg):
    """The record of two tracks of one utterance (F frames each)."""
    f_ref, f_deg = np.asarray(f_ref, np.float64), np.asarray(f_deg, np.float64)
    F = len(f_ref)
    vr, vd = f_ref > 0, f_deg > 0
    both = vr & vd
    rec = {"rmse_cents": np.nan, "gpe": np.nan, "vde": np.nan, "frames": F, "both_voiced": int(both.sum()), "ref_voiced": int(vr.sum()),
           "deg_voiced": int(vd.sum()), "status": SHORT}
    if F == 0:
        return rec
    rec["vde"] = float((vr != vd).sum()) / F
    rec["status"] = UNVOICED
    if both.any():
        ratio = f_deg[both] / f_ref[both]
        rec["rmse_cents"] = float(np.sqrt(np.mean((1200.0 * np.log2(ratio)) ** 2)))
        rec["gpe"] = float((np.abs(ratio - 1.0) > 0.2).sum()) / int(both.sum())
        rec["status"] = OK
    return rec


def measure(clean, degraded, **cfg):
    """The record of a pair of waveforms: both tracked in float64, the tracks rounded to float32 as the library's outputs are."""
    fr, fd = track(clean, **cfg)[0], track(degraded, **cfg)[0]
    return compare(fr.astype(np.float32), fd.astype(np.float32))
