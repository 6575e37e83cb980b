"""The oracle of tests/test_mel_nnls.py: the non-negative mel inversion of include/fastdiff_hip_ext.h (fd_mel_to_linear_nnls) restated in
numpy -- the iteration in float64, the same iteration with every rounding in float32 (the yardstick the device bars are multiples of),
the step bound from numpy.linalg.eigvalsh, and the exact optimum from scipy.optimize.nnls.  Pure numpy / scipy, no GPU.

    x_0 = max(0, P g);  y_0 = x_0
    k < n:  r = A y_k - g;  x_{k+1} = max(0, y_k - s A^T r);  y_{k+1} = x_{k+1} + beta_k (x_{k+1} - x_k)
    amp = max(1e-10, x_n)

A [80, 513] and P [513, 80] are the float32 matrices the device is given, g [80, T] the float32 values it forms (g_of: float64 10^x or
e^x rounded once; the device's exp10f / expf may differ from that by an ulp, which the tests that need g exactly read back from the device).
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import mel_frontend  # noqa: E402

MELS, BINS, FLOOR = 80, 513, 1e-10
POWER_ITERS, MARGIN = 200, 1.01
OK, EMPTY, NONFINITE = 0, 1, 2


def default_bank(variant="pwg"):
    """The front-end's default bank [80, 513] float32 (oracle/mel_frontend.mel_basis)."""
    fb = mel_frontend.mel_basis() if variant == "pwg" else mel_frontend.mel_basis(fmin=mel_frontend.TACO_FMIN, fmax=mel_frontend.TACO_FMAX)
    return np.ascontiguousarray(fb.astype(np.float32))


def dense_bank(seed=17):
    """A dense bank of mixed sign: 80 x 513 N(0, 1) / 16, float32."""
    return np.ascontiguousarray((np.random.default_rng(seed).standard_normal((MELS, BINS)) / 16.0).astype(np.float32))


def pinv(bank):
    return np.ascontiguousarray(np.linalg.pinv(np.asarray(bank, np.float64)).astype(np.float32))


def g_of(mel, variant="pwg"):
    """g(mel) float32 [80, T]: float64 10^x / e^x, rounded once."""
    m = np.asarray(mel, np.float64)
    return (np.power(10.0, m) if variant == "pwg" else np.exp(m)).astype(np.float32)


def lambda_max(bank):
    A = np.asarray(bank, np.float64)
    return float(np.linalg.eigvalsh(A @ A.T)[-1])


def step_bound(bank):
    """The header's L restated: 200 power iterations on the Gram matrix from v_j = 1 + j / 80, then 1.01 times the Rayleigh quotient."""
    A = np.asarray(bank, np.float64)
    G = A @ A.T
    v = 1.0 + np.arange(MELS) / MELS
    for _ in range(POWER_ITERS):
        w = G @ v
        n = np.sqrt(w @ w)
        if not n > 0:
            break
        v = w / n
    return MARGIN * float(v @ (G @ v) / (v @ v))


@functools.lru_cache(maxsize=None)
def betas(n):
    """beta_k, k < n: float64, and the float32 table the device is given"""
    t, out = 1.0, np.empty(n, np.float64)
    for k in range(n):
        t1 = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out[k] = (t - 1.0) / t1
        t = t1
    b32 = out.astype(np.float32)
    out.setflags(write=False)
    b32.setflags(write=False)
    return out, b32


def solve(bank, P, g, n_iters, L, dtype=np.float64):
    """x_n [513, T] before the floor.  dtype float64: the definition, with the float32 step and betas the device uses; float32: the
    same with every operation rounded to float32."""
    dt = np.dtype(dtype)
    A, Pm, gv = np.asarray(bank, np.float32).astype(dt), np.asarray(P, np.float32).astype(dt), np.asarray(g, np.float32).astype(dt)
    s = dt.type(np.float32(1.0 / L))
    beta = betas(max(int(n_iters), 1))[1].astype(dt)
    x = np.maximum(dt.type(0), Pm @ gv)
    y = x.copy()
    At = np.ascontiguousarray(A.T)
    for k in range(int(n_iters)):
        r = A @ y - gv
        xn = np.maximum(dt.type(0), y - s * (At @ r))
        y = xn + beta[k] * (xn - x)
        x = xn
    return x


def amplitudes(x):
    return np.maximum(np.asarray(x, np.float64), FLOOR)


def residual(bank, amp, g):
    """|| A amp - g ||_2 / || g ||_2 per frame, float64"""
    A, a, gv = np.asarray(bank, np.float64), np.asarray(amp, np.float64), np.asarray(g, np.float64)
    return np.sqrt(((A @ a - gv) ** 2).sum(0)) / np.sqrt((gv ** 2).sum(0))


def record(bank, amp, g):
    """(resid, norm) of an item, float64: Frobenius over its frames"""
    A, a, gv = np.asarray(bank, np.float64), np.asarray(amp, np.float64), np.asarray(g, np.float64)
    n2 = (gv ** 2).sum()
    return float(np.sqrt(((A @ a - gv) ** 2).sum() / n2)), float(np.sqrt(n2))


def image_gap(bank, a, b, g):
    """|| A (a - b) ||_2 / || g ||_2 per frame, float64"""
    A = np.asarray(bank, np.float64)
    return np.sqrt(((A @ (np.asarray(a, np.float64) - np.asarray(b, np.float64))) ** 2).sum(0)) / np.sqrt((np.asarray(g, np.float64) ** 2).sum(0))


def optimum(bank, g):
    """The exact optimum's relative residual per frame (scipy.optimize.nnls, float64)."""
    from scipy.optimize import nnls
    A, gv = np.asarray(bank, np.float64), np.asarray(g, np.float64)
    return np.array([nnls(A, gv[:, t], maxiter=20000)[1] / np.sqrt((gv[:, t] ** 2).sum()) for t in range(gv.shape[1])])


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def _signal(frames):
    n = mel_frontend.HOP * (frames - 1)
    t = np.arange(n) / mel_frontend.SR
    x = sum(0.3 / h * np.sin(2 * np.pi * 185.0 * h * t + 0.7 * h) for h in range(1, 30))
    return x + 0.01 * np.random.default_rng(5).standard_normal(n)


@functools.lru_cache(maxsize=None)
def mels(kind, variant="pwg", bank_id="default"):
    """The log-mels [80, T] float32 of input `kind` for a bank (banks(bank_id, variant)): "cone" (40 frames: the bank applied to |STFT|
    of a harmonic-plus-noise signal, so a non-negative preimage exists), "noisy" (cone times 10^(0.1 N(0, 1))), "random" (24 frames of
    U(-4, 0.5) in log10: no preimage), "floor" (8 frames of log10 = -6).  Computed once, read-only."""
    log = np.log10 if variant == "pwg" else np.log
    ln10 = 1.0 if variant == "pwg" else np.log(10.0)
    if kind in ("cone", "noisy"):
        S = mel_frontend.stft_mag(_signal(40))
        m = np.asarray(bank(bank_id, variant), np.float64) @ S
        if bank_id == "dense":                                # a mixed-sign bank's image may be negative: the mel of |.|, floored
            m = np.abs(m)
        m = np.maximum(m, 1e-6)
        if kind == "noisy":
            m = m * np.power(10.0, 0.1 * np.random.default_rng(9).standard_normal(m.shape))
        out = log(m)
    elif kind == "random":
        out = np.random.default_rng(3).uniform(-4.0, 0.5, (MELS, 24)) * ln10
    elif kind == "floor":
        out = np.full((MELS, 8), -6.0) * ln10
    else:
        raise KeyError(kind)
    out = np.ascontiguousarray(out.astype(np.float32))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def bank(bank_id="default", variant="pwg"):
    fb = dense_bank() if bank_id == "dense" else default_bank(variant)
    fb.setflags(write=False)
    return fb


@functools.lru_cache(maxsize=None)
def bank_pinv(bank_id="default", variant="pwg"):
    P = pinv(bank(bank_id, variant))
    P.setflags(write=False)
    return P
