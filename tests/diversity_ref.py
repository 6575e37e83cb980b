"""Oracle of fastdiff_amd.diversity and fd_bins_pass, written from the text of the issue and of include/fastdiff_hip_ext.h: the
standardisation in float32 exactly as the header says, then float64 distances, Lloyd's iteration and the NDB / JSD statistics of
Richardson & Weiss 2018.  Plain numpy and math; nothing here imports the package.

    standardise(x, shift, scale)     z = fl(fl(x - shift) * scale) in float32
    finite_rows(z)                   rows whose z are all finite
    dist64(z, c)                     [N, K] float64 squared distances over the float32 z
    assign64(z, c)                   the nearest bin per row (lowest k of equal ones), -1 for a row that is not finite
    assign32(z, c)                   the header's float32 form (h_k - dot_k with fma chains), same conventions
    tau(z, c, a)                     the header's rounding bound per row for the assignment a, and d64(a) - min_k d64(k)
    lloyd_pass(z, c, prev)           one pass in float64 -> dict(assign, counts, inertia, moved, nonfinite, empty, centroids)
    update_bound(z, a, K, chunk)     (float64 mean [K, D], bound [K, D]) of a float32 sum in chunks of `chunk` rows
    ndb_jsd(r, q, alpha)             the statistics with plain loops
"""
import math

import numpy as np

U = 2.0 ** -24


def standardise(x, shift=None, scale=None):
    x = np.asarray(x, np.float32)
    if shift is None:
        return x.copy()
    with np.errstate(all="ignore"):
        return ((x - np.asarray(shift, np.float32)).astype(np.float32) * np.asarray(scale, np.float32)).astype(np.float32)


def finite_rows(z):
    return np.isfinite(z).all(1)


def dist64(z, c):
    z64, c64 = np.asarray(z, np.float64), np.asarray(c, np.float64)
    out = np.empty((z64.shape[0], c64.shape[0]))
    for k in range(c64.shape[0]):
        t = z64 - c64[k]
        out[:, k] = (t * t).sum(1)
    return out


def assign64(z, c):
    ok = finite_rows(z)
    a = np.full(z.shape[0], -1, np.int64)
    if ok.any():
        a[ok] = np.argmin(dist64(z[ok], c), axis=1)
    return a


def _fma32(a, b, acc):
    """fma(a, b, acc) of float32 operands: the product is exact in float64, the sum is rounded to float64 and then to float32 (a double
    rounding that differs from the fused operation only when the float64 sum lies within 2^-29 relative of a float32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def scores32(z, c):
    """s [N, K] float32: s_k = fl(h_k - dot_k), h_k = fl(0.5 * fma chain of c_kd^2), dot_k = fma chain of c_kd z_d in ascending d."""
    z, c = np.asarray(z, np.float32), np.asarray(c, np.float32)
    h = np.zeros(c.shape[0], np.float32)
    dot = np.zeros((z.shape[0], c.shape[0]), np.float32)
    for d in range(c.shape[1]):
        h = _fma32(c[:, d], c[:, d], h)
        dot = _fma32(c[None, :, d], z[:, None, d], dot)
    h = (np.float32(0.5) * h).astype(np.float32)
    return (h[None, :] - dot).astype(np.float32)


def assign32(z, c):
    ok = finite_rows(z)
    a = np.full(z.shape[0], -1, np.int64)
    if ok.any():
        a[ok] = np.argmin(scores32(z[ok], c), axis=1)
    return a


def tau(z, c, a):
    """(tau [n], excess [n]) over the rows with a >= 0: tau = 2 g (E_a + E_best), E_k = ||c_k||^2 / 2 + sum_d |z_d| |c_kd|, g = n u / (1 -
    n u), n = D + 2; excess = d64(a) - min_k d64(k)."""
    a = np.asarray(a)
    rows = np.nonzero(a >= 0)[0]
    z64, c64 = np.asarray(z, np.float64)[rows], np.asarray(c, np.float64)
    d = dist64(z64, c64)
    best = np.argmin(d, axis=1)
    n = c64.shape[1] + 2
    g = n * U / (1.0 - n * U)
    E = 0.5 * (c64 * c64).sum(1)[None, :] + np.abs(z64) @ np.abs(c64).T
    i = np.arange(rows.size)
    return 2.0 * g * (E[i, a[rows]] + E[i, best]), d[i, a[rows]] - d[i, best]


def inertia64(z, c, a):
    a = np.asarray(a)
    rows = a >= 0
    t = np.asarray(z, np.float64)[rows] - np.asarray(c, np.float64)[a[rows]]
    return float((t * t).sum())


def means64(z, a, c):
    """[K, D] float64 means of the rows of every bin; an empty bin keeps c[k]."""
    z64, out = np.asarray(z, np.float64), np.asarray(c, np.float64).copy()
    for k in range(out.shape[0]):
        rows = a == k
        if rows.any():
            out[k] = z64[rows].sum(0) / rows.sum()
    return out


def lloyd_pass(z, c, prev=None):
    a = assign64(z, c)
    K = c.shape[0]
    counts = np.bincount(a[a >= 0], minlength=K).astype(np.int64)
    return {"assign": a, "counts": counts, "inertia": inertia64(z, c, a), "moved": -1 if prev is None else int((a != np.asarray(prev)).sum()),
            "nonfinite": int((a < 0).sum()), "empty": int((counts == 0).sum()), "centroids": means64(z, a, c)}


def update_bound(z, a, c, chunk):
    """(mean [K, D] float64, bound [K, D]): |float32-summed mean - mean| <= chunk * u * mean|z_d| over the bin (a float32 sum of at most
    `chunk` terms per chunk, the chunks added in float64) plus the quotient's one rounding u |mean|."""
    mean = means64(z, a, c)
    bound = np.zeros_like(mean)
    absz = np.abs(np.asarray(z, np.float64))
    for k in range(mean.shape[0]):
        rows = a == k
        if rows.any():
            bound[k] = chunk * U * absz[rows].mean(0) + U * np.abs(mean[k])
    return mean, bound


def ndb_jsd(r, q, alpha=0.05):
    r, q = [float(v) for v in r], [float(v) for v in q]
    n_r, n_q, K = sum(r), sum(q), len(r)
    ndb, z, different, jsd = 0, [], [], 0.0
    for k in range(K):
        P, Q = r[k] / n_r, q[k] / n_q
        p = (r[k] + q[k]) / (n_r + n_q)
        se = math.sqrt(p * (1.0 - p) * (1.0 / n_r + 1.0 / n_q))
        zk = (P - Q) / se if se > 0 else 0.0
        dk = se > 0 and math.erfc(abs(zk) / math.sqrt(2.0)) < alpha
        z.append(zk)
        different.append(dk)
        ndb += int(dk)
        M = 0.5 * (P + Q)
        if P > 0:
            jsd += 0.5 * P * math.log(P / M)
        if Q > 0:
            jsd += 0.5 * Q * math.log(Q / M)
    return {"ndb": ndb, "ndb_over_k": ndb / K, "jsd": jsd, "z": np.array(z), "different": np.array(different, bool)}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def gaussians(seed, N, D, K, spread=1.5):
    """Overlapping clusters in raw units (per-feature offset and scale, so that the standardisation does something):
    -> (x [N, D] float32, shift [D], scale [D] float32, centroids [K, D] float32 in z units)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (K, D))
    z = centres[rng.integers(0, K, N)] + rng.normal(0.0, 1.0, (N, D))
    mu, sd = rng.uniform(-5.0, 5.0, D), rng.uniform(0.5, 3.0, D)
    x = (z * sd + mu).astype(np.float32)
    shift, scale = mu.astype(np.float32), (1.0 / sd).astype(np.float32)
    cent = (centres + rng.normal(0.0, 0.3, (K, D))).astype(np.float32)
    return x, shift, scale, cent


def blobs(seed, N, D, K, sep=20.0):
    """K blobs of unit variance whose centres lie sep * sqrt 2 apart (sep along one axis each), of unequal sizes, rows shuffled:
    -> (x [N, D] float32, labels [N])."""
    assert K <= D
    rng = np.random.default_rng(seed)
    w = np.arange(1, K + 1, dtype=np.float64)
    labels = rng.choice(K, size=N, p=w / w.sum())
    labels[:K] = np.arange(K)
    centres = np.zeros((K, D))
    centres[np.arange(K), np.arange(K)] = sep
    x = (centres[labels] + rng.normal(0.0, 1.0, (N, D))).astype(np.float32)
    return x, labels
