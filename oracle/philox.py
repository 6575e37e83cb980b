"""Host twin of the on-device noise generator (fdk::philox_normal4, fastdiff_amd/csrc/fd_device.h): Philox4x32-10 + Box-Muller.

numpy only; test infrastructure.  Written from the published definition of Philox4x32-10 (Salmon et al., "Parallel random numbers: as
easy as 1, 2, 3", SC'11; its Random123 known-answer vectors are in tests/test_device_noise.py) and from DESIGN.md 3.4.

One call of the generator gives four N(0,1) draws ("a float4") from
    counter = (idx4 lo, idx4 hi ^ uid lo, stream, 0x5EED ^ uid hi)        key = (seed lo, seed hi)
where idx4 is a float4 index, uid the utterance's noise stream id (0 without ids), stream the executed step index k for z_k and
0xFFFFFFFF for x_T.  Each output word r becomes the float32 uniform  u = ((float)(r >> 8) + 0.5f) * 2^-24  -- the sum is rounded
to float32 (25 significant bits, ties to even), so u lies in [2^-25, 1.0] with both ends reached -- and
    (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(6.2831855f * u1)          (z2, z3) the same from (u2, u3).
u0 >= 2^-25 bounds |z| by sqrt(50 ln 2) = 5.887.

Index convention of the whole-tensor helpers x_T() and z(), for a batch [B, L] of L samples per utterance (L is the caller's length,
never a frame bucket):
  * without uids:  sample (b, t) has flat index i = b * L + t;  idx4 = i >> 2, component = i & 3, uid = 0
    (when L % 4 != 0 a float4 straddles two utterances);
  * with uids:     idx4 = (t >> 2) + offs[b], component = t & 3, uid = uids[b];  offs[b] is the float4 offset of a window's first
    sample inside its utterance (0 for a whole utterance).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
X_T_STREAM = 0xFFFFFFFF
Z_MAX = 5.887                      # sqrt(50 ln 2) = 5.88705 to four figures: the bar of the element-wise tests
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_TWO_PI_F32 = np.float32(6.283185307179586)      # 6.2831855f, what the device multiplies by


def _u64(v):
    """Python ints (any size: taken mod 2^64) or integer arrays -> uint64 array."""
    if isinstance(v, (int, np.integer)):
        return np.asarray(int(v) & 0xFFFFFFFFFFFFFFFF, np.uint64)
    a = np.asarray(v)
    if a.dtype == object:
        return np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in a.ravel()], np.uint64).reshape(a.shape)
    return a.astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on uint64 arrays that hold 32-bit words (broadcast against each other); returns the four output words."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for i in range(10):
        p0, p1 = _MUL0 * c0, _MUL1 * c2                   # 32 x 32 -> 64 bit products: no overflow in uint64
        rk0, rk1 = (k0 + np.uint64(i * _W0)) & M32, (k1 + np.uint64(i * _W1)) & M32
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ rk0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ rk1, p0 & M32
    return c0, c1, c2, c3


def u_from_word(r):
    """A 32-bit output word -> the float32 uniform, every step in float32 as on the device."""
    hi = (_u64(r) >> np.uint64(8)).astype(np.float32)      # < 2^24: exact
    return (hi + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def words(seed, stream, idx4, uid=0):
    """The four Philox output words of float4 `idx4` (arrays broadcast)."""
    seed, idx4, uid, stream = _u64(seed), _u64(idx4), _u64(uid), _u64(stream)
    s32 = np.uint64(32)
    return philox4x32_10(idx4 & M32, (idx4 >> s32) ^ (uid & M32), stream, np.uint64(0x5EED) ^ (uid >> s32), seed & M32, seed >> s32)


def uniforms(seed, stream, idx4, uid=0):
    """[..., 4] float32: u0..u3 exactly as philox_normal4 forms them."""
    return np.stack([u_from_word(r) for r in words(seed, stream, idx4, uid)], axis=-1)


def normal4_from_uniforms(u):
    """Box-Muller in float64 on float32 uniforms [..., 4] and on the float32 product 6.2831855f * u: what is left between this and the
    device is the rounding of logf, sqrtf, sincosf and of the final multiply."""
    u = np.asarray(u, np.float32)
    out = np.empty(u.shape, np.float64)
    for j in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., j].astype(np.float64)))
        a = (_TWO_PI_F32 * u[..., j + 1]).astype(np.float64)        # float32 * float32 -> float32, then widened
        out[..., j], out[..., j + 1] = r * np.cos(a), r * np.sin(a)
    return out


def normal4_f64(seed, stream, idx4, uid=0):
    """[..., 4] float64: the four draws of float4 `idx4`."""
    return normal4_from_uniforms(uniforms(seed, stream, idx4, uid))


def _tensor(seed, stream, B, L, uids, offs):
    B, L = int(B), int(L)
    if uids is None:
        assert offs is None, "window offsets need stream ids"
        q = normal4_f64(seed, stream, np.arange((B * L + 3) // 4, dtype=np.uint64))
        return q.reshape(-1)[: B * L].reshape(B, 1, L)                             # flat: component i & 3 of float4 i >> 2
    assert len(uids) == B and (offs is None or len(offs) == B)
    out = np.empty((B, 1, L), np.float64)
    n4 = (L + 3) // 4
    for b in range(B):
        first = 0 if offs is None else int(offs[b])
        q = normal4_f64(seed, stream, np.arange(first, first + n4, dtype=np.uint64), int(uids[b]))
        out[b, 0] = q.reshape(-1)[:L]
    return out


def x_T(seed, B, L, uids=None, offs=None):
    """[B, 1, L] float64: the initial noise of a call with x_T = None (stream 0xFFFFFFFF)."""
    return _tensor(seed, X_T_STREAM, B, L, uids, offs)


def z(seed, k, B, L, uids=None, offs=None):
    """[B, 1, L] float64: the noise added after executed step k (stream k)."""
    return _tensor(seed, int(k), B, L, uids, offs)
