"""The float64 oracle of the mel-cepstral distortion (include/fastdiff_hip_ext.h: "Mel-cepstral distortion with time alignment").

cepstra: the float64 log-mel oracle of the mel tests (oracle/mel_frontend.py) as natural logarithms through the orthonormal DCT-II,
coefficients 1 .. n_coef.  dtw: the header's recurrence with its tie rule, vectorised over anti-diagonals (every cell of an anti-diagonal
depends on the two before it only), carrying the path's cells and diagonal steps forward AND keeping the directions, so that the
back-tracked path is there to compare with.  Everything in float64 on whatever costs it is given.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import mel_frontend as mf      # noqa: E402

OK, SHORT, NONFINITE = 0, 1, 2
MELS, HOP, DEFAULT_COEF, MAX_COEF = 80, 256, 13, 40
K_DB = 10.0 * np.sqrt(2.0) / np.log(10.0)


def frames(n):
    return 1 + n // HOP


def dct_matrix(n=MELS):
    """[n, n]: row d = the orthonormal DCT-II basis vector d (row 0: 1 / sqrt(n))."""
    j = np.arange(n)
    m = np.sqrt(2.0 / n) * np.cos(np.pi * np.arange(n)[:, None] * (j[None, :] + 0.5) / n)
    m[0] = np.sqrt(1.0 / n)
    return m


def log_mel(wav, variant="pwg", bank=None):
    """[80, T] natural log of the front-end's floored mel, float64.  bank: a filter bank [80, 513] instead of the default."""
    wav = np.asarray(wav, np.float64)
    if variant == "tacotron":
        b = mf.mel_basis(fmin=mf.TACO_FMIN, fmax=mf.TACO_FMAX) if bank is None else np.asarray(bank, np.float64)
        return np.log(np.maximum(mf.TACO_CLIP, b @ mf.stft_mag_reflect(wav)))
    b = mf.mel_basis() if bank is None else np.asarray(bank, np.float64)
    return np.log(10.0) * np.log10(np.maximum(mf.EPS, b @ mf.stft_mag(wav)))


def cepstra(wav, n_coef=DEFAULT_COEF, variant="pwg", bank=None):
    """[T, n_coef] float64."""
    return (dct_matrix()[1: n_coef + 1] @ log_mel(wav, variant, bank)).T


def costs(a, b):
    """[Ta, Tb] Euclidean distances of the rows of a and b, float64, from the differences."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))


def dtw(cost):
    """cost [Ta, Tb] -> dict: acc [Ta, Tb] the accumulated matrix, cost, path_len, n_diag (carried forward), dirs [Ta, Tb] (0 diagonal,
    1 from i - 1, 2 from j - 1; (0, 0): 0).  Ties to the first of (diagonal, i - 1, j - 1)."""
    c = np.asarray(cost, np.float64)
    Ta, Tb = c.shape
    inf = np.inf
    acc = np.full((Ta + 1, Tb + 1), inf)                  # one border row and column of "absent"
    ln = np.zeros((Ta + 1, Tb + 1), np.int64)
    nd = np.zeros((Ta + 1, Tb + 1), np.int64)
    dirs = np.zeros((Ta, Tb), np.int8)
    acc[1, 1] = c[0, 0]
    ln[1, 1] = 1
    for s in range(1, Ta + Tb - 1):
        i = np.arange(max(0, s - Tb + 1), min(Ta, s + 1))
        j = s - i
        I, J = i + 1, j + 1
        dg, up, lf = acc[I - 1, J - 1], acc[I - 1, J], acc[I, J - 1]
        d = np.zeros(len(i), np.int8)
        best = dg.copy()
        m = up < best
        d[m], best[m] = 1, up[m]
        m = lf < best
        d[m], best[m] = 2, lf[m]
        acc[I, J] = c[i, j] + best
        pi, pj = I - (d != 2), J - (d != 1)
        ln[I, J] = ln[pi, pj] + 1
        nd[I, J] = nd[pi, pj] + (d == 0)
        dirs[i, j] = d
    return {"acc": acc[1:, 1:], "cost": float(acc[Ta, Tb]), "path_len": int(ln[Ta, Tb]), "n_diag": int(nd[Ta, Tb]), "dirs": dirs}


def backtrack(dirs):
    """The path [(i, j)] from (0, 0) to the end that the directions describe."""
    i, j = dirs.shape[0] - 1, dirs.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        d = dirs[i, j]
        i, j = i - (d != 2), j - (d != 1)
        path.append((i, j))
    return path[::-1]


def align_from_path(path, Ta):
    """For each i the smallest j with (i, j) on the path (the reference's align_from_distances)."""
    out = np.full(Ta, -1, np.int64)
    for i, j in path[::-1]:
        out[i] = j
    return out


def path_cost(cost, path):
    return float(sum(cost[i, j] for i, j in path))


def is_monotone_path(path, Ta, Tb):
    if path[0] != (0, 0) or path[-1] != (Ta - 1, Tb - 1):
        return False
    return all((i1 - i0, j1 - j0) in ((1, 1), (1, 0), (0, 1)) for (i0, j0), (i1, j1) in zip(path, path[1:]))


def brute_force(cost):
    """The smallest cost over every monotone path, by enumeration."""
    Ta, Tb = cost.shape
    best = [np.inf]

    def go(i, j, acc):
        acc += cost[i, j]
        if (i, j) == (Ta - 1, Tb - 1):
            best[0] = min(best[0], acc)
            return
        if i + 1 < Ta and j + 1 < Tb:
            go(i + 1, j + 1, acc)
        if i + 1 < Ta:
            go(i + 1, j, acc)
        if j + 1 < Tb:
            go(i, j + 1, acc)

    go(0, 0, 0.0)
    return best[0]


def measure(clean, degraded, n_coef=DEFAULT_COEF, variant="pwg"):
    """The record of one pair from the waveforms, float64 throughout."""
    ca, cb = cepstra(clean, n_coef, variant), cepstra(degraded, n_coef, variant)
    r = dtw(costs(ca, cb))
    T = min(len(ca), len(cb))
    lin = np.sqrt(((ca[:T] - cb[:T]) ** 2).sum(-1)).mean()
    return {"mcd_dtw": K_DB * r["cost"] / r["path_len"], "mcd_linear": K_DB * lin, "cost": r["cost"], "path_len": r["path_len"], "n_diag": r["n_diag"],
            "frames_clean": len(ca), "frames_degraded": len(cb), "status": OK}
