"""Float64 oracle of Griffin-Lim as include/fastdiff_hip_ext.h ("Griffin-Lim") defines it: numpy only, test infrastructure.

N = 1024, hop = 256, the periodic Hann window; frames t < n_frames of an item <-> L = 256 (n_frames - 1) samples.
    stft(y)        [513, T] complex: frames of y zero-padded by 512 on both sides (librosa.stft(center=True, pad_mode="constant"))
    istft(C, n)    [256 (n - 1)]: irfft of every frame (the imaginary parts of bins 0 and 512 ignored), windowed, overlap-added, divided by
                   the overlap-added squared window, the 512 padded samples cut off (librosa.istft, torch.istft(center=True))
    griffin_lim(A, theta0, n_iters)   C_0 = A e^(i theta0); X = stft(y), C = A X / |X| (X = 0: C = A), y = istft(C)
    philox_angles(seed, uid, T)       the random start: theta = 6.2831855f u, u = oracle.philox.u_from_word of word k % 4 of generator call
                   129 t + k // 4 on stream FD_GL_PHILOX_STREAM with id uid
    inconsistency(y, A)               || |stft(y)| - A ||_F / || A ||_F
    mel_to_linear(mel, P, variant)    max(1e-10, P @ g(mel)), g = 10^x ("pwg") or e^x ("tacotron")
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import philox  # noqa: E402  (oracle/philox.py)

N, HOP, BINS, PAD = 1024, 256, 513, 512
PHILOX_STREAM = 0xFFFFFFF8
CALLS_PER_FRAME = 129
OK, SHORT, SILENT, NONFINITE = 0, 1, 2, 3
WINDOW = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)
_TWO_PI_F32 = np.float32(6.283185307179586)


def samples(frames):
    return -1 if frames < 2 else HOP * (frames - 1)


def stft(y):
    """y [L], L = 256 (T - 1) -> X [513, T] complex128"""
    y = np.asarray(y, np.float64)
    assert y.ndim == 1 and y.size % HOP == 0 and y.size >= HOP
    T = 1 + y.size // HOP
    yp = np.concatenate([np.zeros(PAD), y, np.zeros(PAD)])
    frames = np.stack([yp[HOP * t: HOP * t + N] for t in range(T)])
    return np.fft.rfft(frames * WINDOW, axis=1).T


def envelope(n_frames):
    """sum_t w^2[m - 256 t] over the n_frames frames, for every padded position m < 1024 + 256 (n_frames - 1)"""
    e = np.zeros(N + HOP * (n_frames - 1))
    for t in range(n_frames):
        e[HOP * t: HOP * t + N] += WINDOW ** 2
    return e


def istft(C, n_frames=None):
    """C [513, T] complex, the first n_frames frames of it -> y [256 (n_frames - 1)] float64"""
    C = np.asarray(C, np.complex128)
    n = C.shape[1] if n_frames is None else int(n_frames)
    assert C.shape[0] == BINS and 2 <= n <= C.shape[1]
    C = C[:, :n].copy()
    C[0] = C[0].real
    C[BINS - 1] = C[BINS - 1].real
    f = np.fft.irfft(C.T, n=N, axis=1) * WINDOW
    y = np.zeros(N + HOP * (n - 1))
    for t in range(n):
        y[HOP * t: HOP * t + N] += f[t]
    L = HOP * (n - 1)
    return (y / np.where(envelope(n) > 0, envelope(n), 1.0))[PAD: PAD + L]


def rephase(A, X):
    mag = np.abs(X)
    safe = np.where(mag > 0, mag, 1.0)
    return np.where(mag > 0, A * X / safe, A.astype(np.complex128))


def griffin_lim(A, theta0, n_iters, n_frames=None, trace=False):
    """A, theta0 [513, T] -> y after n_iters iterations (trace: also the list of sc after 0 .. n_iters iterations)"""
    A = np.asarray(A, np.float64)
    n = A.shape[1] if n_frames is None else int(n_frames)
    A = A[:, :n]
    y = istft(A * np.exp(1j * np.asarray(theta0, np.float64)[:, :n]))
    scs = [inconsistency(y, A)] if trace else None
    for _ in range(int(n_iters)):
        y = istft(rephase(A, stft(y)))
        if trace:
            scs.append(inconsistency(y, A))
    return (y, scs) if trace else y


def inconsistency(y, A):
    A = np.asarray(A, np.float64)
    X = np.abs(stft(y))
    A = A[:, :X.shape[1]]
    return float(np.sqrt(((X - A) ** 2).sum() / (A ** 2).sum()))


def philox_positions(T):
    """(pos [513, T] uint64, word [513]) of the draw of every (bin, frame)"""
    k = np.arange(BINS, dtype=np.uint64)[:, None]
    t = np.arange(T, dtype=np.uint64)[None, :]
    return t * np.uint64(CALLS_PER_FRAME) + (k >> np.uint64(2)), (np.arange(BINS) & 3)


def philox_uniforms(seed, uid, T):
    """[513, T] float32: the uniform of every (bin, frame)"""
    pos, word = philox_positions(T)
    w = np.stack(philox.words(seed, PHILOX_STREAM, pos, uid))            # [4, 513, T]
    r = np.take_along_axis(w, word[None, :, None].repeat(T, axis=2), axis=0)[0]
    return philox.u_from_word(r)


def philox_angles(seed, uid, T):
    """[513, T] float32 angles: 6.2831855f u, the product rounded to float32"""
    return (_TWO_PI_F32 * philox_uniforms(seed, uid, T)).astype(np.float32)


def status(A, n_frames):
    if n_frames < 2:
        return SHORT
    a = np.asarray(A)[:, :n_frames]
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        return NONFINITE
    return SILENT if not np.any(a) else OK


def mel_to_linear(mel, P, variant="pwg"):
    """mel [80, T], P [513, 80] -> (amplitudes [513, T] float64, the bound's scale sum_j |P_kj| g(mel_j))"""
    g = np.power(10.0, np.asarray(mel, np.float64)) if variant == "pwg" else np.exp(np.asarray(mel, np.float64))
    P = np.asarray(P, np.float64)
    return np.maximum(1e-10, P @ g), np.abs(P) @ g
